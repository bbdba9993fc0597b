// The body of a res4 bottleneck and the head of the next one in ONE kernel (gfx950), ResNet-50/101
// [detectron2 BottleneckBlock, recalled; built by build_dafne_resnet_fpn_backbone, backbone/fpn.py:58-91]:
//
//     T = relu(conv2_b(U) + bias2)                3x3, 256 -> 256, pad 1   (U = relu(conv1_b(.)), the block's first 1x1)
//     Y = relu(conv3_b(T) + bias3 + X)            1x1, 256 -> 1024, X = the block's shortcut (identity or projection)
//     Z = relu(conv1_{b+1}(Y) + bias1)            1x1, 1024 -> 256
//
// T never leaves the CU: the 3x3's output tile (128 px x 256 ch bf16 = 64 KB) IS the LDS operand of conv3's GEMM, and a
// 256-channel chunk of Y is the LDS operand of conv1' before (and while) its rows go to HBM.
//
// Structure (8 waves, one workgroup per CU, a workgroup owns a 4 x 32 pixel tile and ALL channels):
//   phase A (3x3): the (4+2) x (32+2) input patch is DMA'd into LDS for all 256 channels (four 64-channel slabs of
//     26 KB, [pixel][128 B] with the 16-byte chunk XOR (patch column >> 1) & 7: conflict-free ds_read_b128 at any tap offset) and
//     STAYS there -- the nine taps read their B fragments from it at tap-dependent pixel offsets (LDS-staged im2col), so
//     the 144 k16 steps of the layer run without a single barrier between them except one after the first slab.  The
//     weights stream L2 -> REGISTERS: a wave owns 32 output channels and all 128 pixels, so every 1-KiB weight fragment feeds
//     4 MFMAs and is fetched by exactly one wave (fragment-major packing, ring of 8 steps, hand-counted vmcnt).  K order =
//     (64-channel slab, kh, kw, k16 step): the order of conv_igemm_kernel, so T is bit-identical to the separate launch.
//   phase B (round 6: a TWO-HALF PING-PONG; rounds 3-5 ran conv_b2b.hip's lock-step schedule here -- all eight waves in GEMM1,
//     then all in the epilogue with the matrix pipe idle, then all in GEMM2 behind the residual DMA and the Y row stores: 68 k
//     cycles of phase B held 33 k cycles of matrix work).  Per 256-channel chunk c of Y a wave runs four segments, each closed
//     by a workgroup barrier:
//         G1(c)   16 k16 steps   acc1 = W3[c] . T
//         E(c)    the epilogue   y = relu((acc1 + bias3) + x), x and y IN REGISTERS: bf16 -> this wave's 32 channels of the Y
//                                chunk in LDS (the K operand of conv1') and straight to HBM (8 x 16-byte stores per lane); behind
//                                pixel fragment b's stores the same registers are re-loaded with chunk c + 1's shortcut values
//         G2a(c)  8 k16 steps    acc2 += W1[:, c, slabs 0..1] . Y
//         G2b(c)  8 k16 steps    acc2 += W1[:, c, slabs 2..3] . Y
//     and waves 4..7 (the SIMD mates of waves 0..3) run the same program ONE SEGMENT LATER (one extra barrier at entry):
//         segment       4c          4c+1        4c+2        4c+3        4c+4
//         waves 0..3    G1(c)       E(c)        G2a(c)      G2b(c)      G1(c+1)
//         waves 4..7    G2b(c-1)    G1(c)       E(c)        G2a(c)      G2b(c)
//     so an epilogue always runs beside the mate's matrix segment.  Waves 0..3 own slabs 0..1 of every 256-channel output,
//     waves 4..7 slabs 2..3: G2a(c) reads what waves 0..3 wrote in E(c) (segment 4c+1 <  4c+2, 4c+3), G2b(c) what waves 4..7
//     wrote (4c+2 < 4c+3, 4c+4); the next writes of the two buffer halves come in segments 4c+5 / 4c+6, behind every read.
//     The shortcut X does not pass through LDS (rounds 3-5: DMA into the Y buffer, slab by slab behind GEMM2's reads, with
//     barriers; every wait for a weight fragment also waited for those HBM-latency pieces): a lane loads exactly the values
//     of its own accumulator elements, a whole chunk ahead.  For that the output rows of every matrix are PERMUTED inside a
//     wave's 32 (engine.pack_bneck): MFMA row 8g + 4h + i holds channel 16 (g >> 1) + 8h + 4 (g & 1) + i, so the 16 accumulator
//     registers of a lane and pixel fragment are two runs of 8 consecutive channels = two 16-byte pieces of a pixel's row.
//     Every output element is the same sum in the same order as before: bit-identical to the separate launches.
// Ragged tiles (H % 4 or W % 32 != 0): loads are clamped into the buffer; the stores of out-of-image pixels are issued with
// those lanes' EXEC bits off (the instruction count -- and with it the vmcnt bookkeeping -- is the same for every tile).
#include <cstdlib>
#include <type_traits>

#include "common.h"

namespace {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(2))) float f32x2;
typedef __attribute__((ext_vector_type(4))) unsigned u32x4;
typedef __attribute__((ext_vector_type(2))) unsigned u32x2;
typedef __attribute__((address_space(1))) void gvoid;
typedef __attribute__((address_space(3))) void lvoid;

// Tile geometry, a template parameter of the kernel (round 6): TH x 32 output pixels, TH = 4 (128 pixels: a weight fragment feeds four
// MFMAs) or TH = 2 (64 pixels, two MFMAs per fragment) for launches with few tiles -- a res4 block of ONE image is 32 tiles of 4 x 32 on
// 256 CUs; every CU streams the block's 2.2 MB of weights whatever its tile, so the half tile costs twice the L2 -> CU traffic per pixel
// and is chosen only where the CUs would otherwise be idle (dafne_bottleneck_body_hip).  The weight layout does not depend on it.
constexpr int kTW = 32, kPC = kTW + 2;
template <int TH>
struct BN {
    static constexpr int kTH = TH, kPx = TH * kTW;             // output tile
    static constexpr int kPR = TH + 2;                         // input patch rows
    static constexpr int kPPieces = (kPR * kPC + 7) / 8;       // DMA pieces of 8 px x 128 B per slab: 26 (TH 4) / 17 (TH 2)
    static constexpr int kPP = (kPPieces + 7) / 8;             // pieces per wave and slab: 4 / 3
    static constexpr int kPSlab = kPPieces * 1024;
    static constexpr int kSlab = kPx * 128;                    // one 64-channel slab of the tile: 16 / 8 KB
    static constexpr int kBuf = 4 * kSlab;                     // 256 channels
    // LDS map.  The patch is dead when T is written.
    static constexpr int kOffY = 0;                            // phase B: the Y chunk (K operand of conv1')
    static constexpr int kOffT = kBuf;                         // T tile
    static constexpr int kOffPatch = 3 * kSlab;                // phase A only: [4 slabs][patch px][128 B]
    static constexpr int kOffBias = kOffPatch + 4 * kPSlab;    // fp32 [256 conv2 | 1024 conv3 | 256 conv1 | 2 x 256 spare]
    static constexpr int kSmemTotal = kOffBias + 8 * 1024;
    static_assert(kOffPatch + 4 * kPSlab >= kOffT + kBuf && kSmemTotal <= 160 * 1024, "LDS budget");
    static constexpr int kPF = kPx / 32;                       // pixel fragments per wave
    static constexpr int kRL = kPx / 16;                       // quad-layout row instructions per wave and 256-channel chunk (16 px each)
    static constexpr int kTrickle = 3 * kPP;                   // patch slabs 1..3: one piece per wave and step 0 .. kTrickle - 1
    // k16 steps of A fragments in flight per wave (32 registers).  (Round 6: 16 for the half tile -- it has the registers -- changed
    // nothing: 27.7 us per block alone, 0.894 against 0.908 ms for the 22 blocks of one image in the plan.)
    static constexpr int kRing = 8;
};
constexpr int kCM = 256, kCB = 1024, kChunks = kCB / 256;
constexpr int kNW = 8, kNT = 512;
constexpr int kStepsA = 9 * (kCM / 16);                // 144 k16 steps of the 3x3
constexpr int kStepsB = 2 * kChunks * 16;              // 128 k16 steps of conv3 + conv1'
constexpr int kSteps = kStepsA + kStepsB;
constexpr int kWABytes = kNW * kStepsA * 1024;         // phase A weights: [8 waves][144 steps][64 lanes][8]
constexpr int kPhaseBytes = kNW * 16 * 1024;           // one GEMM of phase B: [8 waves][16 steps][64 lanes][8]
constexpr int kRes0 = 60, kResStride = 4;              // the first shortcut chunk: one register load per lane at steps 60, 64, ..
constexpr int kDumpBytes = 128 * kCB * 2;              // scratch the ABI asks for (rounds 3-5: rows of out-of-image pixels; now timing stamps only)

struct BneckDev {
    const char* in;      // bf16 [N, H+2, W+2, 256]   U
    const char* res;     // bf16 [N, H+2, W+2, 1024]  X
    const char* wf;      // bf16 phase A [8][144][64][8] | phase B [8 GEMMs][8 waves][16 steps][64][8]; rows permuted (see above)
    const float* b2;     // [256]
    const float* b3;     // [1024]
    const float* b1;     // [256]
    char* out;           // bf16 [N, H+2, W+2, 1024]  Y
    char* next;          // bf16 [N, H+2, W+2, 256]   Z
    char* dump;          // >= kDumpBytes
    int N, H, W, tiles_x, tiles_per_img, tiles;
    unsigned max_pix;    // N * (H+2) * (W+2) - 1
};

__device__ __forceinline__ int xcd_remap(int bid, int nwg) {
    const int xcd = bid & 7, idx = bid >> 3;
    const int q = nwg >> 3, r = nwg & 7;
    const int start = xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
    return start + idx;
}

__device__ __forceinline__ unsigned pack_bf16(float a, float b) {
    typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
    f32x2 v = {a, b};
    bf16x2 r = __builtin_convertvector(v, bf16x2);
    return __builtin_bit_cast(unsigned, r);
}

// Vector-memory program order of a wave: bias piece (1 DMA) | patch slab 0 (4 DMA) | A(0) .. A(7) | then for every k16
// step s = 0 .. 271 (0..143 phase A; 144 + 32 c + i = step i of chunk c: i < 16 G1, 16..23 G2a, 24..31 G2b):
//   [wait A(s)] MFMAs | A(s + 8) if it exists | bn_post(s) more operations:
//     phase A: one patch piece of slabs 1..3 at steps 0..11; one 16-byte register load of the first shortcut chunk at steps
//              60, 64, .., 88 (HBM is idle while every CU is in phase A);
//     phase B: behind the last step of G1(c), in E(c): 8 row stores of Y and (c < 3) the 8 register loads of chunk c + 1's
//              shortcut values.
// bn_wait(j) = number of those instructions issued after A(j) and before the wait for it: vmcnt retires in order, so
// `s_waitcnt vmcnt(bn_wait(j))` is exactly "A(j) and everything older has landed".  The shortcut loads of chunk c sit in front
// of A(144 + 32 c - 8): the first step of G2b(c - 1) already waits for them, a whole G1 ahead of their use in E(c).
template <int TH>
constexpr int bn_post(int s) {
    constexpr int kRL = BN<TH>::kRL;
    if (s < kStepsA)
        return (s < BN<TH>::kTrickle ? 1 : 0) + ((s >= kRes0 && s < kRes0 + kRL * kResStride && (s - kRes0) % kResStride == 0) ? 1 : 0);
    const int j = s - kStepsA, i = j & 31, c = j >> 5;
    return i == 15 ? kRL + (c + 1 < kChunks ? kRL : 0) : 0;
}
template <int TH>
constexpr int bn_wait(int j) {
    int n = 0;
    constexpr int kRing = BN<TH>::kRing;
    if (j < kRing) {
        n += kRing - 1 - j;                                    // A(j+1 .. 7)
        for (int s = 0; s < j; s++) n += 1 + bn_post<TH>(s);
    } else {
        n += bn_post<TH>(j - kRing);                           // the operations right behind A(j) at the end of step j - 8
        for (int s = j - kRing + 1; s < j; s++) n += (s + kRing < kSteps ? 1 : 0) + bn_post<TH>(s);
    }
    return n;
}
// spot checks (hand-counted, 4 x 32 tiles): steady state 7; the trickle adds one per step; the 16 operations of an epilogue
static_assert(bn_wait<4>(0) == 7 && bn_wait<4>(1) == 8 && bn_wait<4>(7) == 14 && bn_wait<4>(8) == 15 && bn_wait<4>(12) == 15 && bn_wait<4>(13) == 14 &&
              bn_wait<4>(20) == 7 && bn_wait<4>(61) == 8 && bn_wait<4>(68) == 9 && bn_wait<4>(100) == 7 && bn_wait<4>(kStepsA + 7) == 7 &&
              bn_wait<4>(kStepsA + 15) == 7 && bn_wait<4>(kStepsA + 16) == 23 && bn_wait<4>(kStepsA + 23) == 23 && bn_wait<4>(kStepsA + 24) == 7 &&
              bn_wait<4>(kStepsA + 96 + 16) == 15 && bn_wait<4>(kStepsA + 96 + 24) == 7 && bn_wait<4>(kStepsA + 127) == 0 &&
              bn_wait<2>(9) == 15 && bn_wait<2>(10) == 14 && bn_wait<2>(kStepsA + 16) == 15 && bn_wait<2>(kStepsA + 96 + 16) == 11,
              "vmcnt bookkeeping");

// ---- the 16x16x32 form (conv_bneck_kernel<HEAD, TH, true>, dafne_bottleneck_body16_hip): the same tile, LDS layout, weight stream
// and ping-pong with v_mfma_f32_16x16x32_bf16 -- half the accumulator traffic per flop (profiles/NOTES_r06.md; the towers' form:
// conv.hip, conv3x3_rp_kernel<GNIN, true>).  A k32 group = the former k16 steps 2m, 2m + 1 (phase A: of one (slab, tap)).  Fragment
// F(2m + cb) = output channels of MFMA rows 16 cb .. 16 cb + 15 of the wave x the 32 k of group m (lane: row lane & 15, k 8 (lane >> 4)
// .. + 8); a B fragment = 16 pixels x those 32 k (lane: pixel lane & 15, the same k).  Step 2m + h multiplies BOTH fragments of its group
// with pixel fragments kPF h .. kPF h + kPF - 1 (16 tile pixels each: tile row p >> 1, columns 16 (p & 1) ..), so a fragment lives for
// two steps, and the ring of this form is TEN fragments deep: F(s + 9) is requested at the end of step s into slot (s + 9) % 10, the slot
// of the fragment that died one step ago, and the even step of a pair waits for the pair's younger fragment, requested eight steps
// before -- the cover of the 32x32x16 form, and its wait counts (7 in the steady state).  Measured in the plan, where a block's weights
// come cold: a ring of 8 (five to six steps of cover) cost 4 % per launch, 10 and 12 are level with the 32x32x16 form
// (profiles/NOTES_bneck_mfma16.md).  Still one 1-KiB load per step, and the same bn_post operations behind it.
// Rows: a lane holds rows 4 (lane >> 4) + i of a 16-row fragment, so row 4a + i of fragment cb holds channel 8a + 4 cb + i of the wave's
// 32 (engine.pack_bneck16): the lane's 4 + 4 values of a pixel fragment are ONE run of 8 consecutive channels -- the 16-byte piece
// lane >> 4 of the pixel's 64 bytes.
constexpr int kRing16 = 10, kDist16 = kRing16 - 1;
template <int TH>
constexpr int bn_wait16(int s) {                       // even s: the operations issued after F(s + 1) and before the wait of step s
    int n = 0;
    if (s + 1 < kDist16) {
        n += kDist16 - 1 - (s + 1);                            // F(s + 2 .. kDist16 - 1) of the prologue
        for (int u = 0; u < s; u++) n += 1 + bn_post<TH>(u);
    } else {
        n += bn_post<TH>(s + 1 - kDist16);                     // the operations right behind F(s + 1) at the end of step s + 1 - kDist16
        for (int u = s + 2 - kDist16; u < s; u++) n += (u + kDist16 < kSteps ? 1 : 0) + bn_post<TH>(u);
    }
    return n;
}
static_assert(bn_wait16<4>(0) == 7 && bn_wait16<4>(2) == 9 && bn_wait16<4>(4) == 11 && bn_wait16<4>(6) == 13 && bn_wait16<4>(8) == 15 &&
              bn_wait16<4>(20) == 7 && bn_wait16<4>(kStepsA + 16) == 23 && bn_wait16<4>(kStepsA + 22) == 23 && bn_wait16<4>(kStepsA + 24) == 7 &&
              bn_wait16<4>(kSteps - 2) == 0 && bn_wait16<2>(kStepsA + 16) == 15 && bn_wait16<2>(kStepsA + 96 + 16) == 11,
              "vmcnt bookkeeping (16x16x32 form)");

template <int I, int N, class F>
__device__ __forceinline__ void static_for(F&& f) {
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        static_for<I + 1, N>(f);
    }
}

// A fragment of k16 step J: one coalesced 1-KiB load per wave, L2 -> registers.  Inline asm: the compiler would sink visible
// loads to their uses and wait for each; readiness is tracked by hand (bn_wait).
template <int J, int kRing>
__device__ __forceinline__ void bn_load(bf16x8 (&ar)[kRing], const char* wf, unsigned voffA, unsigned voffB) {
    if constexpr (J < kStepsA) {
        const char* sb = wf + (size_t)J * 1024;
        // "+v": ONE register per ring slot from the zero-initialisation on (an output-only operand lets the compiler move the
        // value between registers -- e.g. inside the plain-C++ epilogues -- while the load is in flight: conv.hip rp_load)
        asm volatile("global_load_dwordx4 %0, %1, %2" : "+v"(ar[J % kRing]) : "v"(voffA), "s"(sb) : "memory");
    } else if constexpr (J < kSteps) {
        constexpr int jb = J - kStepsA;
        const char* sb = wf + (size_t)kWABytes + (size_t)(jb >> 4) * kPhaseBytes + (jb & 15) * 1024;
        asm volatile("global_load_dwordx4 %0, %1, %2" : "+v"(ar[J % kRing]) : "v"(voffB), "s"(sb) : "memory");
    }
}
// the PF B fragments of phase-A step J (patch rows kh .. kh + PF - 1 at tap column kw, chunk kc of slab sl; PSLAB = the slab's bytes):
// inline asm, completion is awaited by the caller (lgkmcnt)
template <int J, int PF, int PSLAB>
__device__ __forceinline__ void bn_bread(bf16x8 (&b)[PF], const unsigned (&pb)[3], unsigned lds_base) {
    constexpr int sl = J / 36, t = J % 36, kh = t / 12, kw = (t >> 2) % 3, kc = t & 3;
    const unsigned ad = lds_base + ((pb[kw] ^ (unsigned)(kc << 5)) + (unsigned)(sl * PSLAB));
    constexpr int o0 = (kh + 0) * kPC * 128, o1 = (kh + 1) * kPC * 128, o2 = (kh + 2) * kPC * 128, o3 = (kh + 3) * kPC * 128;
    if constexpr (PF == 4) {
        asm volatile("ds_read_b128 %0, %4 offset:%5\n\tds_read_b128 %1, %4 offset:%6\n\tds_read_b128 %2, %4 offset:%7\n\tds_read_b128 %3, %4 offset:%8"
                     : "=&v"(b[0]), "=&v"(b[1]), "=&v"(b[2]), "=&v"(b[3])
                     : "v"(ad), "n"(o0), "n"(o1), "n"(o2), "n"(o3)
                     : "memory");
    } else {
        static_assert(PF == 2, "2 or 4 pixel fragments");
        asm volatile("ds_read_b128 %0, %2 offset:%3\n\tds_read_b128 %1, %2 offset:%4"
                     : "=&v"(b[0]), "=&v"(b[1])
                     : "v"(ad), "n"(o0), "n"(o1)
                     : "memory");
    }
}

// the same in the 16x16x32 form: step J = group J >> 1 (k32 group kc2 of slab sl at tap (kh, kw)) x pixel fragments PF (J & 1) .. + PF - 1:
// fragment f = patch row kh + (PF / 2) (J & 1) + (f >> 1), column half f & 1 (16 pixels = 2048 B on: the swizzle of column q + 16 is
// that of q)
template <int J, int PF, int PSLAB>
__device__ __forceinline__ void bn_bread16(bf16x8 (&b)[PF], const unsigned (&pb)[3], unsigned lds_base) {
    constexpr int sl = J / 36, t = J % 36, kh = t / 12, kw = (t >> 2) % 3, kc2 = (t >> 1) & 1;
    const unsigned ad = lds_base + ((pb[kw] ^ (unsigned)(kc2 << 6)) + (unsigned)(sl * PSLAB));
    constexpr int r0 = kh + (PF / 2) * (J & 1);
    constexpr int o0 = r0 * kPC * 128, o1 = o0 + 2048, o2 = (r0 + 1) * kPC * 128, o3 = o2 + 2048;
    static_assert(o3 <= 65535, "ds_read immediate");
    if constexpr (PF == 4) {
        asm volatile("ds_read_b128 %0, %4 offset:%5\n\tds_read_b128 %1, %4 offset:%6\n\tds_read_b128 %2, %4 offset:%7\n\tds_read_b128 %3, %4 offset:%8"
                     : "=&v"(b[0]), "=&v"(b[1]), "=&v"(b[2]), "=&v"(b[3])
                     : "v"(ad), "n"(o0), "n"(o1), "n"(o2), "n"(o3)
                     : "memory");
    } else {
        static_assert(PF == 2, "2 or 4 pixel fragments");
        asm volatile("ds_read_b128 %0, %2 offset:%3\n\tds_read_b128 %1, %2 offset:%4"
                     : "=&v"(b[0]), "=&v"(b[1])
                     : "v"(ad), "n"(o0), "n"(o1)
                     : "memory");
    }
}

// phase B: the PF B fragments (pixel fragments STRIDE B apart: 32 pixels; 16x16x32 form: 16) of k step ST of the slab at byte offset
// OFF of the buffer at BUF
template <int BUF, int OFF, int ST, int PF, int STRIDE = 4096>
__device__ __forceinline__ void bn_bread_b(bf16x8 (&b)[PF], const unsigned (&bs)[4], unsigned lds_base) {
    const unsigned ad = lds_base + (unsigned)BUF + bs[ST];
    constexpr int o = OFF;
    static_assert(o + 3 * STRIDE <= 65535, "ds_read immediate");
    if constexpr (PF == 4) {
        asm volatile("ds_read_b128 %0, %4 offset:%5\n\tds_read_b128 %1, %4 offset:%6\n\tds_read_b128 %2, %4 offset:%7\n\tds_read_b128 %3, %4 offset:%8"
                     : "=&v"(b[0]), "=&v"(b[1]), "=&v"(b[2]), "=&v"(b[3])
                     : "v"(ad), "n"(o), "n"(o + STRIDE), "n"(o + 2 * STRIDE), "n"(o + 3 * STRIDE)
                     : "memory");
    } else {
        asm volatile("ds_read_b128 %0, %2 offset:%3\n\tds_read_b128 %1, %2 offset:%4"
                     : "=&v"(b[0]), "=&v"(b[1])
                     : "v"(ad), "n"(o), "n"(o + STRIDE)
                     : "memory");
    }
}
// the caller's wait for the fragments of the current step: all but the PF youngest LDS operations
template <int PF, bool LAST>
__device__ __forceinline__ void bn_bwait(bf16x8 (&b)[PF]) {
    if constexpr (PF == 4) {
        if constexpr (LAST) asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(b[0]), "+v"(b[1]), "+v"(b[2]), "+v"(b[3]) :: "memory");
        else asm volatile("s_waitcnt lgkmcnt(4)" : "+v"(b[0]), "+v"(b[1]), "+v"(b[2]), "+v"(b[3]) :: "memory");
    } else {
        if constexpr (LAST) asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(b[0]), "+v"(b[1]) :: "memory");
        else asm volatile("s_waitcnt lgkmcnt(2)" : "+v"(b[0]), "+v"(b[1]) :: "memory");
    }
}

template <int J, int TH>
__device__ __forceinline__ void bn_wait_for(bf16x8 (&ar)[BN<TH>::kRing]) {
    constexpr int kWaitN = bn_wait<TH>(J), kRing = BN<TH>::kRing;
    static_assert(kWaitN < 64, "vmcnt is a 6-bit counter");
    asm volatile("s_waitcnt vmcnt(%1)" : "+v"(ar[J % kRing]) : "n"(kWaitN) : "memory");
}

template <int J, int TH>
__device__ __forceinline__ void bn_wait16_for(bf16x8 (&ar)[kRing16]) {
    static_assert((J & 1) == 0, "the even step of a pair waits");
    constexpr int kWaitN = bn_wait16<TH>(J), kRing = kRing16;
    static_assert(kWaitN < 64, "vmcnt is a 6-bit counter");
    asm volatile("s_waitcnt vmcnt(%2)" : "+v"(ar[J % kRing]), "+v"(ar[(J + 1) % kRing]) : "n"(kWaitN) : "memory");
}

// HEAD = false (the stage's last block: no next conv1): GEMM2 and the Z rows are skipped; the weight stream still
// walks the (zero) conv1' fragments -- the vmcnt bookkeeping is one schedule for both forms.
// M16: the 16x16x32 form (above).
template <bool HEAD, int TH, bool M16>
__global__ void __launch_bounds__(512, 2) conv_bneck_kernel(BneckDev P) {
    typedef BN<TH> Geo;
    constexpr int kTH = Geo::kTH, kPx = Geo::kPx, kPPieces = Geo::kPPieces, kPP = Geo::kPP, kPSlab = Geo::kPSlab, kSlab = Geo::kSlab;
    constexpr int kOffY = Geo::kOffY, kOffT = Geo::kOffT, kOffPatch = Geo::kOffPatch, kOffBias = Geo::kOffBias;
    constexpr int kPF = Geo::kPF, kRL = Geo::kRL, kTrickle = Geo::kTrickle, kRing = M16 ? kRing16 : Geo::kRing;
    static_assert(kPx == kTH * kTW, "tile");
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // a lane's fragment row (its pixel in a B fragment) and its 8-wide piece of the fragment's k (16x16x32 form: 16 rows, 4 pieces)
    const int frow = M16 ? (lane & 15) : (lane & 31), half = M16 ? (lane >> 4) : (lane >> 5);
    const unsigned lds_base = (unsigned)(size_t)(__attribute__((address_space(3))) char*)lds;

    const int tile = xcd_remap(blockIdx.x, P.tiles);
    const int img = tile / P.tiles_per_img;
    const int tt = tile - img * P.tiles_per_img;
    const int ty = tt / P.tiles_x, tx = tt - ty * P.tiles_x;
    const int row0 = ty * kTH, col0 = tx * kTW;
    const int Wp = P.W + 2;

    // ---- patch DMA map: piece pc = 8 consecutive patch pixels (patch pixel pp = p * 34 + q <-> input pixel
    // (row0 - 1 + p, col0 - 1 + q)); wave w moves pieces w, w + 8, .. (kPP of every slab; a wave without a last piece re-loads the
    // slab's last one: every wave issues the same number of DMAs)
    size_t pofs[kPP];
    unsigned pdst[kPP];
#pragma unroll
    for (int ii = 0; ii < kPP; ii++) {
        int pc = wave + kNW * ii;
        pc = pc < kPPieces ? pc : kPPieces - 1;
        const int pp = pc * 8 + (lane >> 3);
        const int p = pp / kPC, q = pp - p * kPC;
        unsigned g = (unsigned)((img * (P.H + 2) + row0 + p) * Wp + col0 + q);
        g = g < P.max_pix ? g : P.max_pix;                       // ragged tiles reach past the image (and the buffer)
        pofs[ii] = (size_t)g * (kCM * 2) + (unsigned)(((lane & 7) ^ ((q >> 1) & 7)) * 16);      // swizzle by patch COLUMN
        pdst[ii] = (unsigned)(kOffPatch + pc * 1024);
    }
    auto patch_piece = [&](int sl, int ii) {
        __builtin_amdgcn_global_load_lds((gvoid*)(P.in + pofs[ii] + sl * 128), (lvoid*)(lds + pdst[ii] + sl * kPSlab), 16, 0, 0);
    };

    // ---- HBM <-> LDS in QUAD layout: instruction k (0..7) of a wave moves the wave's 64 bytes (its 32 channels) of the 16 tile
    // pixels 16 k + (lane >> 2): lane & 3 = the 16-byte piece -- 4 consecutive lanes = 64 consecutive bytes of a pixel's row (a
    // lane-per-pixel access straight from the accumulator layout is 64 separate 16-byte requests per instruction: the CU's
    // address path then takes 64 cycles per instruction and an epilogue 6-8 k cycles; measured, round 6).  Pixel 16 k + (lane >> 2)
    // = tile row k >> 1, column 16 (k & 1) + (lane >> 2): the row part of an address is wave-uniform (a scalar base per tile
    // row), the column part one register per k & 1.  Loads are clamped into the image; stores of out-of-image pixels are issued
    // with those lanes' EXEC bits off (the instruction count -- vmcnt bookkeeping -- is the same for every tile).
    const unsigned lq = (unsigned)(wave * 64 + (lane & 3) * 16);
    unsigned qcz[2], qcx[2];                               // column part: Z rows (512 B per pixel), X / Y rows (2048 B per pixel)
    unsigned long long colm[2];
#pragma unroll
    for (int kk = 0; kk < 2; kk++) {
        int c = col0 + 16 * kk + (lane >> 2);
        colm[kk] = __builtin_amdgcn_ballot_w64(c < P.W);
        c = c < P.W ? c : P.W - 1;
        qcz[kk] = (unsigned)(c + 1) * (unsigned)(kCM * 2) + lq;
        qcx[kk] = (unsigned)(c + 1) * (unsigned)(kCB * 2) + lq;
    }
    auto row_pix = [&](int kr) {                           // first haloed pixel of tile row kr (clamped), wave-uniform
        int r = row0 + kr;
        r = r < P.H ? r : P.H - 1;
        return (size_t)((img * (P.H + 2) + r + 1) * Wp);
    };
    auto row_mask = [&](int k) -> unsigned long long { return row0 + (k >> 1) < P.H ? colm[k & 1] : 0ull; };
    // shortcut values of the chunk ahead in quad layout: rs[k], loaded by inline asm ("+v": one register set for the whole kernel),
    // valid behind the weight waits that cover them (see bn_post)
    u32x4 rs[kRL];
#pragma unroll
    for (int k = 0; k < kRL; k++) rs[k] = u32x4{};
    auto res_load = [&](auto C, auto K) {
        constexpr int c = decltype(C)::value, k = decltype(K)::value;
        u32x4(&rr)[kRL] = rs;                   // (a non-dependent use: a generic lambda captures the array only through one)
        const unsigned vo = qcx[k & 1];
        const char* xb = P.res + row_pix(k >> 1) * (size_t)(kCB * 2);
        // default cache policy.  (Rounds 4-5 marked the shortcut DMA non-temporal: +0.45 %.  Here a 128-byte line of X is read by TWO
        // waves, 64 bytes each, at different moments: with `nt` the second one fetched it from HBM again -- 108.6 against 101.1 MB
        // fetched per block, 70.6 against 67.7 us, round 6)
        asm volatile("global_load_dwordx4 %0, %1, %2 offset:%3" : "+v"(rr[k]) : "v"(vo), "s"(xb), "n"(c * 512) : "memory");
    };
    // a 16-byte row store with the lanes of out-of-image pixels switched off (all 64 lanes are active around it: the kernel has no
    // divergent control flow); the instruction is issued -- and counted by vmcnt -- whatever the mask
    auto row_store = [&](char* base, unsigned vo, unsigned long long m, const u32x4& v, auto OFF) {
        constexpr int off = decltype(OFF)::value;
        asm volatile("s_mov_b64 exec, %3\n\tglobal_store_dwordx4 %0, %1, %2 offset:%4\n\ts_mov_b64 exec, -1"
                     :: "v"(vo), "v"(v), "s"(base), "s"(m), "n"(off) : "memory");
    };

    // ---- B fragment offsets
    // phase B: k16 step s inside a slab, pixel fragment 0 of a [128 px][128 B] slab
    unsigned bs[4];
#pragma unroll
    for (int s = 0; s < 4; s++) bs[s] = (unsigned)(frow * 128 + ((((M16 ? 4 : 2) * s + half) ^ ((frow >> 1) & 7)) * 16));      // (16x16x32 form: k32 groups 0, 1)
    // phase A: patch row p (0..5) at tap column kw (0..2): pixel p * 34 + q, q = kw + frow; k16 step kc reads the 16-byte
    // chunk (2 kc + half) ^ sw, sw = (q >> 1) & 7 (the row pitch is even: a swizzle by COLUMN is conflict-free like one by
    // pixel index, and independent of the patch row).  That is  (pb[kw] ^ (kc << 5)) + p * 34 * 128  with
    // pb[kw] = q * 128 | ((half ^ (sw & 1)) << 4) | ((sw >> 1) << 5)   (bits 5..6 of q * 128 are zero)
    unsigned pb[3];
#pragma unroll
    for (int kw = 0; kw < 3; kw++) {
        const int q = kw + frow;
        const int sw = (q >> 1) & 7;
        // (16x16x32 form: the 32-channel group kc2 reads chunk (4 kc2 + half) ^ sw, i.e. (pb[kw] ^ (kc2 << 6)) + p * 34 * 128)
        pb[kw] = M16 ? (unsigned)(kOffPatch + q * 128 + ((half ^ (sw & 3)) << 4) + ((sw >> 2) << 6))
                     : (unsigned)(kOffPatch + q * 128 + ((half ^ (sw & 1)) << 4) + ((sw >> 1) << 5));
    }

    // ---- A operand: L2 -> registers through inline asm, ring of 8 k16 steps
    const unsigned voffA = (unsigned)(wave * kStepsA * 1024 + lane * 16);
    const unsigned voffB = (unsigned)(wave * 16 * 1024 + lane * 16);
    bf16x8 ar[kRing];
#pragma unroll
    for (int k = 0; k < kRing; k++) ar[k] = bf16x8{};
    auto load_step = [&](auto J) { bn_load<decltype(J)::value, kRing>(ar, P.wf, voffA, voffB); };
    auto wait_step = [&](auto J) {
        constexpr int j = decltype(J)::value;
        if constexpr (!M16) bn_wait_for<j, TH>(ar);
        else if constexpr ((j & 1) == 0) bn_wait16_for<j, TH>(ar);
    };
    constexpr int kDist = M16 ? kDist16 : kRing;           // a fragment is requested kDist steps ahead

    // 64 accumulator registers per GEMM: kPF fragments of 32 x 32, or 2 kPF pixel fragments x 2 channel halves of 16 x 16
    // (h[2 p + cb]: pixel fragment p, MFMA rows 16 cb ..)
    f32x16 acc1[M16 ? 1 : kPF], acc2[M16 ? 1 : kPF];
    f32x4 h1[M16 ? 4 * kPF : 1], h2[M16 ? 4 * kPF : 1];
    auto zero_acc = [&](f32x16 (&a)[M16 ? 1 : kPF], f32x4 (&h)[M16 ? 4 * kPF : 1]) {
        if constexpr (M16) {
#pragma unroll
            for (int b = 0; b < 4 * kPF; b++) h[b] = f32x4{0.f, 0.f, 0.f, 0.f};
        } else {
#pragma unroll
            for (int b = 0; b < kPF; b++)
#pragma unroll
                for (int k = 0; k < 16; k++) a[b][k] = 0.f;
        }
    };
    // the matrix instructions of step J on the B fragments in `bf`: one weight fragment x kPF pixel fragments of 32, or (16x16x32 form)
    // the group's two fragments x kPF pixel fragments of 16
    auto mma = [&](f32x16 (&a)[M16 ? 1 : kPF], f32x4 (&h)[M16 ? 4 * kPF : 1], const bf16x8 (&bf)[kPF], auto J) {
        constexpr int j = decltype(J)::value;
        const bf16x8(&ring)[kRing] = ar;
        if constexpr (M16) {
            constexpr int jb = j & ~1, p0 = kPF * (j & 1);
#pragma unroll
            for (int f = 0; f < kPF; f++)
#pragma unroll
                for (int cb = 0; cb < 2; cb++)
                    h[2 * (p0 + f) + cb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ring[(jb + cb) % kRing], bf[f], h[2 * (p0 + f) + cb], 0, 0, 0);
        } else {
#pragma unroll
            for (int b = 0; b < kPF; b++) a[b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ring[j % kRing], bf[b], a[b], 0, 0, 0);
        }
    };

    auto barrier = [&]() {
        __builtin_amdgcn_sched_barrier(0);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
    };
    // ---- epilogues, in the accumulator layout.  A lane holds, of pixel fragment b, channels 8 half + 16 run + 0..7 of its
    // wave's 32 (run = 0, 1) in acc[b][8 run .. 8 run + 7] -- one 16-byte piece of the pixel's row per run.  The expressions
    // are those of the separate kernels: (acc + bias) + residual, max with 0, round to bf16.
    const unsigned lbias_off = lds_base + (unsigned)kOffBias;      // fp32 [256 conv2 | 1024 conv3 | 256 conv1]
    // LDS address of this lane's piece (pixel fragment 0, run 0) in a [4 slabs][128 px][128 B] buffer: slab wave >> 1, 16-byte
    // chunk (4 (wave & 1) + 2 run + half) ^ ((frow >> 1) & 7); run 1 = the address XOR 32, fragment b at + 4096 b
    const unsigned eoff = (unsigned)((wave >> 1) * kSlab + frow * 128 + (((4 * (wave & 1) + half) ^ ((frow >> 1) & 7)) * 16));
    const unsigned ey[2] = {lds_base + (unsigned)kOffY + eoff, lds_base + (unsigned)kOffY + (eoff ^ 32u)};
    // the same 8 KB (this wave's 64 bytes of every pixel row of its slab) in quad layout: pixel lane >> 2 of instruction 0, piece
    // lane & 3 -> chunk (4 (wave & 1) + (lane & 3)) ^ (((lane >> 2) >> 1) & 7); instruction k at + 2048 k (16 pixels on: same swizzle)
    const unsigned ql = lds_base + (unsigned)(kOffY + (wave >> 1) * kSlab + (lane >> 2) * 128 +
                                               (((4 * (wave & 1) + (lane & 3)) ^ ((lane >> 3) & 7)) * 16));
    auto bias16 = [&](int bias0, f32x4 (&bv)[4]) {                 // the lane's 16 biases: bv[2 run], bv[2 run + 1]
        const unsigned bad = lbias_off + (unsigned)((bias0 + wave * 32 + 8 * half) * 4);
        asm volatile("ds_read_b128 %0, %4\n\tds_read_b128 %1, %4 offset:16\n\tds_read_b128 %2, %4 offset:64\n\tds_read_b128 %3, %4 offset:80\n\t"
                     "s_waitcnt lgkmcnt(0)"
                     : "=&v"(bv[0]), "=&v"(bv[1]), "=&v"(bv[2]), "=&v"(bv[3])
                     : "v"(bad)
                     : "memory");
    };
    auto piece = [&](const f32x16& a, auto RUN, const f32x4& blo, const f32x4& bhi, const u32x4& r) -> u32x4 {
        constexpr int run = decltype(RUN)::value;
        u32x4 o;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const unsigned rw = r[k];
            const f32x2 rr = {__uint_as_float(rw << 16), __uint_as_float(rw & 0xffff0000u)};
            const f32x2 aa = {a[8 * run + 2 * k], a[8 * run + 2 * k + 1]};
            const f32x2 bb = {k < 2 ? blo[2 * k] : bhi[2 * k - 4], k < 2 ? blo[2 * k + 1] : bhi[2 * k - 3]};
            const f32x2 v = aa + bb + rr;                           // (acc + bias) + residual  (residual 0 where there is none)
            o[k] = pack_bf16(fmaxf(v[0], 0.f), fmaxf(v[1], 0.f));
        }
        return o;
    };
    auto lds_piece = [&](unsigned ad, const u32x4& v, auto B) {
        constexpr int b = decltype(B)::value;
        asm volatile("ds_write_b128 %0, %1 offset:%2" :: "v"(ad), "v"(v), "n"(b * 4096) : "memory");
    };
    // ---- the same in the 16x16x32 form.  A lane holds, of pixel fragment p (16 pixels), channels 8 half + 0..7 of its wave's 32: h[2 p]
    // the first four, h[2 p + 1] the last four -- ONE 16-byte piece per pixel fragment, at ey[0] + 2048 p (slab wave >> 1, pixel
    // 16 p + frow, chunk (4 (wave & 1) + half) ^ ((frow >> 1) & 7): the expression of eoff with this form's frow and half)
    auto bias8 = [&](int bias0, f32x4 (&bv)[2]) {                  // the lane's 8 biases
        const unsigned bad = lbias_off + (unsigned)((bias0 + wave * 32 + 8 * half) * 4);
        asm volatile("ds_read_b128 %0, %2\n\tds_read_b128 %1, %2 offset:16\n\ts_waitcnt lgkmcnt(0)" : "=&v"(bv[0]), "=&v"(bv[1]) : "v"(bad) : "memory");
    };
    auto piece8 = [&](const f32x4& alo, const f32x4& ahi, const f32x4& blo, const f32x4& bhi, const u32x4& r) -> u32x4 {
        u32x4 o;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const unsigned rw = r[k];
            const f32x2 rr = {__uint_as_float(rw << 16), __uint_as_float(rw & 0xffff0000u)};
            const f32x2 aa = {k < 2 ? alo[2 * k] : ahi[2 * k - 4], k < 2 ? alo[2 * k + 1] : ahi[2 * k - 3]};
            const f32x2 bb = {k < 2 ? blo[2 * k] : bhi[2 * k - 4], k < 2 ? blo[2 * k + 1] : bhi[2 * k - 3]};
            const f32x2 v = aa + bb + rr;                           // (acc + bias) + residual, as above
            o[k] = pack_bf16(fmaxf(v[0], 0.f), fmaxf(v[1], 0.f));
        }
        return o;
    };
    auto lds_piece8 = [&](unsigned ad, const u32x4& v, auto PFR) {
        constexpr int p = decltype(PFR)::value;
        asm volatile("ds_write_b128 %0, %1 offset:%2" :: "v"(ad), "v"(v), "n"(p * 2048) : "memory");
    };
    // the wave's 8 KB of the buffer -> HBM rows in quad layout (LDS operations of one wave execute in order: the pieces this wave
    // wrote a moment ago are read back without a barrier), four instructions per LDS round trip
    auto rows_out = [&](char* base, size_t pix_bytes, const unsigned (&qc)[2], auto OFF) {
        static_for<0, kRL / 4>([&](auto G) {
            constexpr int g = decltype(G)::value;
            const unsigned qa = ql;
            u32x4 v[4];
            asm volatile("ds_read_b128 %0, %4 offset:%5\n\tds_read_b128 %1, %4 offset:%6\n\tds_read_b128 %2, %4 offset:%7\n\tds_read_b128 %3, %4 offset:%8\n\t"
                         "s_waitcnt lgkmcnt(0)"
                         : "=&v"(v[0]), "=&v"(v[1]), "=&v"(v[2]), "=&v"(v[3])
                         : "v"(qa), "n"((4 * g) * 2048), "n"((4 * g + 1) * 2048), "n"((4 * g + 2) * 2048), "n"((4 * g + 3) * 2048)
                         : "memory");
            static_for<0, 4>([&](auto KK) {
                constexpr int k = 4 * g + decltype(KK)::value;
                row_store(base + row_pix(k >> 1) * pix_bytes, qc[k & 1], row_mask(k), v[k & 3], OFF);
            });
        });
    };

#ifdef DAFNE_BNECK_TIMING
    unsigned long long stamp[24], rstamp[24];
    int nstamp = 0;
#define BN_STAMP() (rstamp[nstamp] = __builtin_amdgcn_s_memrealtime(), stamp[nstamp++] = __builtin_amdgcn_s_memtime())
#else
#define BN_STAMP()
#endif
    BN_STAMP();
    // ---- prologue: biases -> LDS by DMA, one 1-KiB piece per wave (wave 0: conv2, 1..4: conv3, 5: conv1, 6..7 re-load
    // conv1 into spare LDS); the oldest vector-memory operation of every wave, so every later wait covers it
    {
        const float* bsrc = wave == 0 ? P.b2 : (wave < 5 ? P.b3 + (wave - 1) * 256 : P.b1);
        __builtin_amdgcn_global_load_lds((gvoid*)(bsrc + lane * 4), (lvoid*)(lds + kOffBias + wave * 1024), 16, 0, 0);
    }
#pragma unroll
    for (int ii = 0; ii < kPP; ii++) patch_piece(0, ii);
    static_for<0, kDist>(load_step);

    // ================================================================ phase A: T = relu(conv2(U) + bias2)
    zero_acc(acc1, h1);
    bf16x8 bfr[2][kPF];
    auto bread_a = [&](bf16x8 (&b)[kPF], auto J) {
        const unsigned(&pq)[3] = pb;              // (non-dependent uses: a generic lambda captures the two only through them)
        const unsigned lb = lds_base;
        if constexpr (M16) bn_bread16<decltype(J)::value, kPF, kPSlab>(b, pq, lb);
        else bn_bread<decltype(J)::value, kPF, kPSlab>(b, pq, lb);
    };
    static_for<0, kStepsA>([&](auto J) {
        constexpr int j = decltype(J)::value;
        wait_step(J);
        if constexpr (j == 0) barrier();             // slab 0 and the biases of every wave have landed
        if constexpr (j == 35) barrier();            // slabs 1..3: every wave passed a wait covering its last piece at step 20
        // the B fragments of step j + 1 are requested before the MFMAs of step j (two register sets; the counted lgkmcnt leaves
        // exactly those four reads in flight)
        if constexpr (j == 0) bread_a(bfr[0], std::integral_constant<int, 0>{});
        if constexpr (j + 1 < kStepsA) {
            bread_a(bfr[(j + 1) & 1], std::integral_constant<int, j + 1>{});
            bn_bwait<kPF, false>(bfr[j & 1]);
        } else {
            bn_bwait<kPF, true>(bfr[j & 1]);
        }
        __builtin_amdgcn_sched_barrier(0);
        mma(acc1, h1, bfr[j & 1], J);
        __builtin_amdgcn_sched_barrier(0);
        load_step(std::integral_constant<int, j + kDist>{});
        if constexpr (j < kTrickle) patch_piece(1 + j / kPP, j % kPP);
        if constexpr (j >= kRes0 && j < kRes0 + kRL * kResStride && (j - kRes0) % kResStride == 0) {
            res_load(std::integral_constant<int, 0>{}, std::integral_constant<int, (j - kRes0) / kResStride>{});
        }
    });
    BN_STAMP();
    barrier();                                       // every wave is done with the patch: T may land on it
    if constexpr (M16) {
        f32x4 bv[2];
        bias8(0, bv);
        const unsigned et = ey[0] + (unsigned)(kOffT - kOffY);
        static_for<0, 2 * kPF>([&](auto PFR) {
            constexpr int p = decltype(PFR)::value;
            lds_piece8(et, piece8(h1[2 * p], h1[2 * p + 1], bv[0], bv[1], u32x4{}), PFR);
        });
    } else {
        f32x4 bv[4];
        bias16(0, bv);
        const unsigned et[2] = {ey[0] + (unsigned)(kOffT - kOffY), ey[1] + (unsigned)(kOffT - kOffY)};
        static_for<0, kPF>([&](auto B) {
            constexpr int b = decltype(B)::value;
            static_for<0, 2>([&](auto RUN) {
                constexpr int run = decltype(RUN)::value;
                lds_piece(et[run], piece(acc1[b], RUN, bv[2 * run], bv[2 * run + 1], u32x4{}), B);
            });
        });
    }
    barrier();
    BN_STAMP();

    // ================================================================ phase B: the two-half ping-pong (see the top of the file)
    zero_acc(acc2, h2);
    // the B fragments of step I of a GEMM segment whose first slab is Q0 of the buffer at BUF: k16 step I & 3 of slab Q0 + (I >> 2); 16x16x32
    // form: k32 group (I >> 1) & 1 of that slab, pixel fragments kPF (I & 1) .. (2048 B apart)
    auto bread_b = [&](bf16x8 (&b)[kPF], auto BUF, auto Q0, auto I) {
        constexpr int buf = decltype(BUF)::value, q = decltype(Q0)::value + (decltype(I)::value >> 2), i = decltype(I)::value;
        const unsigned(&bq)[4] = bs;              // (non-dependent uses: a generic lambda captures the two only through them)
        const unsigned lb = lds_base;
        if constexpr (M16) bn_bread_b<buf, q * kSlab + 2048 * kPF * (i & 1), (i >> 1) & 1, kPF, 2048>(b, bq, lb);
        else bn_bread_b<buf, q * kSlab, i & 3, kPF>(b, bq, lb);
    };
    const bool late = wave >= kNW / 2;               // wave-uniform: waves 4..7 run one segment behind their SIMD mates
    if (late) barrier();
    static_for<0, kChunks>([&](auto C) {
        constexpr int c = decltype(C)::value;
        constexpr int j0 = kStepsA + 32 * c;
        // ---- chunk c's shortcut values: registers (quad layout) -> this wave's own 8 KB of the Y buffer, where E(c) finds them in
        // the accumulator layout.  The 8 KB are free: its readers were G2a(c - 1) / G2b(c - 1) of both halves, at least one barrier
        // ago (see the top of the file).  The values have landed: they are older than A(j0 - 8), which the first step of G2b(c - 1)
        // waited for (chunk 0's: requested in phase A, older than A(96)).  The pin makes the LDS writes depend on an instruction
        // behind those waits.
        if constexpr (kRL == 8) asm volatile("" : "+v"(rs[0]), "+v"(rs[1]), "+v"(rs[2]), "+v"(rs[3]), "+v"(rs[4]), "+v"(rs[5]), "+v"(rs[6]), "+v"(rs[7]) :: "memory");
        else asm volatile("" : "+v"(rs[0]), "+v"(rs[1]), "+v"(rs[2]), "+v"(rs[3]) :: "memory");
        static_for<0, kRL>([&](auto K) {
            constexpr int k = decltype(K)::value;
            const unsigned qa = ql;                 // (non-dependent uses: a generic lambda captures the two only through them)
            const u32x4(&rr)[kRL] = rs;
            asm volatile("ds_write_b128 %0, %1 offset:%2" :: "v"(qa), "v"(rr[k]), "n"(k * 2048) : "memory");
        });
        // ---- G1(c): acc1 = W3[c] . T  (K = 256 over the four slabs of the T tile)
        zero_acc(acc1, h1);
        static_for<0, 16>([&](auto I) {
            constexpr int i = decltype(I)::value;
            constexpr int j = j0 + i;
            constexpr std::integral_constant<int, kOffT> T{};
            constexpr std::integral_constant<int, 0> Q0{};
            wait_step(std::integral_constant<int, j>{});
            if constexpr (i == 0) bread_b(bfr[j & 1], T, Q0, I);
            if constexpr (i + 1 < 16) {
                bread_b(bfr[(j + 1) & 1], T, Q0, std::integral_constant<int, i + 1>{});
                bn_bwait<kPF, false>(bfr[j & 1]);
            } else {
                bn_bwait<kPF, true>(bfr[j & 1]);
            }
            __builtin_amdgcn_sched_barrier(0);
            mma(acc1, h1, bfr[j & 1], std::integral_constant<int, j>{});
            __builtin_amdgcn_sched_barrier(0);
            load_step(std::integral_constant<int, j + kDist>{});
        });
        barrier();
        if constexpr (c == 0) BN_STAMP();
        // ---- E(c): chunk c + 1's shortcut values requested (8 quad loads; the registers were emptied at the top of G1(c)); this
        // wave's 32 channels of Y chunk c: residual pieces from its 8 KB of the Y buffer, y = relu((acc1 + bias3) + x) written over
        // them (the K operand of conv1'), then the 8 KB read back in quad layout and stored
        {
            if constexpr (c + 1 < kChunks) static_for<0, kRL>([&](auto K) { res_load(std::integral_constant<int, c + 1>{}, K); });
            f32x4 bv[M16 ? 2 : 4];
            if constexpr (M16) {
                // four pixel fragments per LDS round trip: their residual pieces in, the y pieces over them
                bias8(256 + c * 256, bv);
                static_for<0, kPF / 2>([&](auto PG) {
                    constexpr int p0 = 4 * decltype(PG)::value;
                    const unsigned e0 = ey[0];
                    u32x4 r[4];
                    asm volatile("ds_read_b128 %0, %4 offset:%5\n\tds_read_b128 %1, %4 offset:%6\n\tds_read_b128 %2, %4 offset:%7\n\tds_read_b128 %3, %4 offset:%8\n\t"
                                 "s_waitcnt lgkmcnt(0)"
                                 : "=&v"(r[0]), "=&v"(r[1]), "=&v"(r[2]), "=&v"(r[3])
                                 : "v"(e0), "n"(p0 * 2048), "n"((p0 + 1) * 2048), "n"((p0 + 2) * 2048), "n"((p0 + 3) * 2048)
                                 : "memory");
                    static_for<0, 4>([&](auto PP) {
                        constexpr int p = p0 + decltype(PP)::value;
                        lds_piece8(ey[0], piece8(h1[2 * p], h1[2 * p + 1], bv[0], bv[1], r[p - p0]), std::integral_constant<int, p>{});
                    });
                });
            } else {
                bias16(256 + c * 256, bv);
                static_for<0, kPF / 2>([&](auto BP) {
                    constexpr int b0 = 2 * decltype(BP)::value;
                    const unsigned e0 = ey[0], e1 = ey[1];
                    u32x4 r[4];
                    asm volatile("ds_read_b128 %0, %4 offset:%6\n\tds_read_b128 %1, %5 offset:%6\n\tds_read_b128 %2, %4 offset:%7\n\tds_read_b128 %3, %5 offset:%7\n\t"
                                 "s_waitcnt lgkmcnt(0)"
                                 : "=&v"(r[0]), "=&v"(r[1]), "=&v"(r[2]), "=&v"(r[3])
                                 : "v"(e0), "v"(e1), "n"(b0 * 4096), "n"((b0 + 1) * 4096)
                                 : "memory");
                    static_for<0, 2>([&](auto BB) {
                        constexpr int b = b0 + decltype(BB)::value;
                        static_for<0, 2>([&](auto RUN) {
                            constexpr int run = decltype(RUN)::value;
                            lds_piece(ey[run], piece(acc1[b], RUN, bv[2 * run], bv[2 * run + 1], r[2 * (b - b0) + run]), std::integral_constant<int, b>{});
                        });
                    });
                });
            }
            rows_out(P.out, (size_t)(kCB * 2), qcx, std::integral_constant<int, c * 512>{});
        }
        barrier();
        if constexpr (c == 0) BN_STAMP();
        // ---- G2a(c), G2b(c): acc2 += W1[:, chunk c] . Y chunk, slabs 0..1 (written by waves 0..3) then slabs 2..3 (waves 4..7)
        static_for<0, 2>([&](auto HH) {
            constexpr int hh = decltype(HH)::value;
            static_for<0, 8>([&](auto I) {
                constexpr int i = decltype(I)::value;
                constexpr int j = j0 + 16 + 8 * hh + i;
                constexpr std::integral_constant<int, kOffY> Y{};
                constexpr std::integral_constant<int, 2 * hh> Q0{};
                wait_step(std::integral_constant<int, j>{});
                if constexpr (HEAD) {
                    if constexpr (i == 0) bread_b(bfr[j & 1], Y, Q0, I);
                    if constexpr (i + 1 < 8) {
                        bread_b(bfr[(j + 1) & 1], Y, Q0, std::integral_constant<int, i + 1>{});
                        bn_bwait<kPF, false>(bfr[j & 1]);
                    } else {
                        bn_bwait<kPF, true>(bfr[j & 1]);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                    mma(acc2, h2, bfr[j & 1], std::integral_constant<int, j>{});
                }
                __builtin_amdgcn_sched_barrier(0);
                load_step(std::integral_constant<int, j + kDist>{});
            });
            // Every wave, also behind G2b(3).  For waves 4..7 that last barrier has no partner among waves 0..3, which are one
            // segment ahead: through their Z rows and gone, or about to be -- s_barrier waits for the surviving waves of a
            // workgroup only.  It is what keeps a late wave's Z pieces (written into slabs 2 / 3 of the Y buffer right below) off
            // the Y chunk its three mates may still be reading in THEIR G2b(3).  (Round 6's first form left it out "for want of a
            // partner": beside memory-bound kernels on other streams the half-tile geometry then produced wrong Z channels 128..255
            // in a third of its launches -- the waves of a half drift apart by whole steps when the weight ring runs dry --,
            // tests/test_gpu_reproducible.py::test_bottleneck_beside_memory_traffic.)
            barrier();
            if constexpr (c == 0) BN_STAMP();
        });
    });
    BN_STAMP();
    // ---- Z = relu(acc2 + bias1): through the wave's 8 KB of the Y buffer (free: its last readers were G2a(3) / G2b(3)) into quad
    // layout and out (waves 0..3 beside G2b(3) of waves 4..7)
    if constexpr (HEAD) {
        if constexpr (M16) {
            f32x4 bv[2];
            bias8(256 + kCB, bv);
            static_for<0, 2 * kPF>([&](auto PFR) {
                constexpr int p = decltype(PFR)::value;
                lds_piece8(ey[0], piece8(h2[2 * p], h2[2 * p + 1], bv[0], bv[1], u32x4{}), PFR);
            });
        } else {
            f32x4 bv[4];
            bias16(256 + kCB, bv);
            static_for<0, kPF>([&](auto B) {
                constexpr int b = decltype(B)::value;
                static_for<0, 2>([&](auto RUN) {
                    constexpr int run = decltype(RUN)::value;
                    lds_piece(ey[run], piece(acc2[b], RUN, bv[2 * run], bv[2 * run + 1], u32x4{}), B);
                });
            });
        }
        rows_out(P.next, (size_t)(kCM * 2), qcz, std::integral_constant<int, 0>{});
    }
#ifdef DAFNE_BNECK_TIMING
    BN_STAMP();
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    BN_STAMP();
    if ((tid & 255) == 0 && blockIdx.x < 32) {       // waves 0 and 4 of the first workgroups, into the scratch area
        unsigned long long* o = (unsigned long long*)P.dump + (blockIdx.x * 2 + (tid >> 8)) * 48;
        for (int k = 0; k < 24; k++) o[k] = k < nstamp ? stamp[k] - stamp[0] : 0;
        for (int k = 0; k < 24; k++) o[24 + k] = k < nstamp ? rstamp[k] - rstamp[0] : 0;      // 100 MHz ticks
    }
#endif
}

template <int TH, bool M16>
int bneck_launch(const BneckDev& D, bool head, hipStream_t stream) {
    DAFNE_MAX_LDS_ONCE(BN<TH>::kSmemTotal, (const void*)conv_bneck_kernel<true, TH, M16>, (const void*)conv_bneck_kernel<false, TH, M16>);
    if (head) hipLaunchKernelGGL((conv_bneck_kernel<true, TH, M16>), dim3(D.tiles), dim3(kNT), BN<TH>::kSmemTotal, stream, D);
    else hipLaunchKernelGGL((conv_bneck_kernel<false, TH, M16>), dim3(D.tiles), dim3(kNT), BN<TH>::kSmemTotal, stream, D);
    return DAFNE_OK;
}

// both exports: m16 = the 16x16x32 form (d_wfrag in engine.pack_bneck16's order)
int bneck_body(const void* d_in, const void* d_res, const void* d_wfrag, const float* d_bias2, const float* d_bias3, const float* d_bias1,
               int n_images, int H, int W, void* d_out, void* d_next, void* d_scratch, size_t scratch_bytes, void* stream, bool m16) {
    const bool head = d_next != nullptr;
    if (!d_in || !d_res || !d_wfrag || !d_bias2 || !d_bias3 || (head && !d_bias1) || !d_out || !d_scratch)
        return dafne::fail(DAFNE_E_INVALID, "bottleneck_body: null argument");
    if (n_images < 1 || H < 1 || W < 1 || (long long)H * W > (1 << 20)) return dafne::fail(DAFNE_E_INVALID, "bottleneck_body: bad size");
    if (scratch_bytes < (size_t)kDumpBytes) return dafne::fail(DAFNE_E_WORKSPACE, "bottleneck_body: scratch %zu < %d", scratch_bytes, kDumpBytes);
    BneckDev D;
    D.in = (const char*)d_in; D.res = (const char*)d_res; D.wf = (const char*)d_wfrag;
    D.b2 = d_bias2; D.b3 = d_bias3; D.b1 = head ? d_bias1 : d_bias2;      // (a valid 1-KB source for the bias DMA; unused without the head)
    D.out = (char*)d_out; D.next = (char*)d_next; D.dump = (char*)d_scratch;
    D.N = n_images; D.H = H; D.W = W;
    D.tiles_x = (W + kTW - 1) / kTW;
    // 4 x 32 tiles; 2 x 32 where the launch would leave seven eighths of the CUs without a tile (one image of a 64 x 64 map: 32 tiles
    // on 256 CUs -> 64 half tiles: 46 -> 28 us per block; same results bit for bit, twice the weight traffic per pixel -- a two-image
    // sub-batch of the timed layout on half tiles cost 0.8 % of the step, so the bound is an eighth, not a quarter).  DAFNE_BNECK_TH =
    // 2 / 4 forces a geometry (tests, A/B runs).
    int cus = 0;
    if (int rc = dafne::device_cus(&cus)) return rc;
    const long long tiles4 = (long long)D.tiles_x * ((H + 3) / 4) * n_images;
    int th = tiles4 * 8 <= cus ? 2 : 4;
    if (const char* e = getenv("DAFNE_BNECK_TH")) {
        const int f = atoi(e);
        if (f == 2 || f == 4) th = f;
    }
    D.tiles_per_img = D.tiles_x * ((H + th - 1) / th);
    const long long tiles = (long long)D.tiles_per_img * n_images;
    const long long pix = (long long)n_images * (H + 2) * (W + 2);
    if (tiles > (1ll << 24) || pix * (kCB * 2) > 0xffffffffll) return dafne::fail(DAFNE_E_UNSUPPORTED, "bottleneck_body: too large");
    D.tiles = (int)tiles;
    D.max_pix = (unsigned)(pix - 1);
    const hipStream_t st = (hipStream_t)stream;
    if (int rc = th == 4 ? (m16 ? bneck_launch<4, true>(D, head, st) : bneck_launch<4, false>(D, head, st))
                         : (m16 ? bneck_launch<2, true>(D, head, st) : bneck_launch<2, false>(D, head, st)))
        return rc;
    return dafne::check_launch("conv_bneck");
}

}  // namespace

extern "C" {

size_t dafne_bottleneck_body_scratch_bytes(void) { return (size_t)kDumpBytes; }

int dafne_bottleneck_body_hip(const void* d_in, const void* d_res, const void* d_wfrag, const float* d_bias2,
                              const float* d_bias3, const float* d_bias1, int n_images, int H, int W, void* d_out,
                              void* d_next, void* d_scratch, size_t scratch_bytes, void* stream) {
    return bneck_body(d_in, d_res, d_wfrag, d_bias2, d_bias3, d_bias1, n_images, H, W, d_out, d_next, d_scratch, scratch_bytes, stream, false);
}

int dafne_bottleneck_body16_hip(const void* d_in, const void* d_res, const void* d_wfrag, const float* d_bias2,
                                const float* d_bias3, const float* d_bias1, int n_images, int H, int W, void* d_out,
                                void* d_next, void* d_scratch, size_t scratch_bytes, void* stream) {
    return bneck_body(d_in, d_res, d_wfrag, d_bias2, d_bias3, d_bias1, n_images, H, W, d_out, d_next, d_scratch, scratch_bytes, stream, true);
}

}  // extern "C"
