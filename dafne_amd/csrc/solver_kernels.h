// Device SGD step over a table of tensors (DESIGN row F14): torch.optim.SGD with momentum (dampening 0, no Nesterov), bit for bit,
// and in the same pass the packed compute copies the engine's launches read -- fp32 biases / GroupNorm affines and the bf16
// convolution weights in pack_conv's K order and in the fragment-major forms -- written where they already lie.
//
// Included at the end of decode.hip, like the other *_kernels.h: that unit is built with -ffp-contract=off -fno-slp-vectorize
// (build.py PER_FILE) and is listed as matrix-free for `build --check` (NO_MATRIX_UNITS), which is what this code needs -- the two
// fmaf below are the only fused operations, as in torch's CPU kernels (g + wd * p and p - lr * buf are fused there, m * buf + g is
// not).
//
// One launch, one workgroup of 256 threads per chunk of the table:
//   elementwise chunk (forms NONE / F32): 1024 consecutive elements, lane-contiguous dword accesses;
//   convolution chunk (form CONV): SGD_ROWS output rows x one 64-channel slab.  Per row that is 64*KH*KW CONTIGUOUS fp32 in each of
//     p / g / buf (OIHW) and as many contiguous bf16 in the plain packed form (slab, kh, kw, channel).  Phase 1 walks the fp32 side in
//     float4 and drops the rounded bf16 into LDS in the packed order; phase 2 reads 16-byte groups (8 K columns of one row) back and
//     stores them row-major into the plain form (1152 contiguous bytes per row for 3x3) and ROW-FASTEST into the fragment forms,
//     where the 16 rows of one K group are 256 contiguous bytes.
// Every output element has exactly one writer; no atomics.
#pragma once
#include "common.h"

#include <string.h>

namespace dafne_sgd {

constexpr int SGD_THREADS = 256;
constexpr int SGD_ELEMS = 1024;        // elements of an elementwise chunk
constexpr int SGD_ROWS = 16;           // output rows of a convolution chunk
constexpr int SGD_MAX_TAPS = 9;        // KH * KW
constexpr int SGD_LDS_ROW = 64 * SGD_MAX_TAPS + 8;        // bf16 per LDS row: 16-byte aligned rows, + 8 spreads the row-fastest reads over banks

struct Chunk {
    int32_t tensor, a, b, reserved;    // elementwise: a = chunk index (elements a*1024 ..); convolution: a = row block, b = slab
};
static_assert(sizeof(Chunk) == 16, "chunk entry");
static_assert(sizeof(dafne_sgd_tensor) == 128, "descriptor layout (include/dafne_amd.h)");

// tensor.to(torch.bfloat16): round to nearest even on the bits (subnormals kept), NaN -> quiet NaN
__device__ __forceinline__ uint16_t bf16_rne(float v) {
    const uint32_t u = __float_as_uint(v);
    if ((u & 0x7fffffffu) > 0x7f800000u) return 0x7fc0;
    return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}

struct StepArgs {
    float neg_lr, momentum, wd;
    int first, zero;
};

__device__ __forceinline__ float sgd_elem(float p, float g, float& buf, const StepArgs& a) {
    const float g1 = a.wd == 0.0f ? g : fmaf(a.wd, p, g);
    float b;
    if (a.first) {
        b = g1;
    } else {
        const float mb = a.momentum * buf;      // rounded ...
        b = mb + g1;                            // ... and rounded again: never one fma (-ffp-contract=off)
    }
    buf = b;
    return fmaf(a.neg_lr, b, p);
}

__global__ __launch_bounds__(SGD_THREADS) void sgd_step_kernel(const dafne_sgd_tensor* __restrict__ tensors, const Chunk* __restrict__ chunks,
                                                                double lr, float momentum, int first, int zero) {
    __shared__ __attribute__((aligned(16))) uint16_t lds[SGD_ROWS * SGD_LDS_ROW];
    const Chunk ck = chunks[blockIdx.x];
    const dafne_sgd_tensor& T = tensors[ck.tensor];
    StepArgs a;
    a.neg_lr = -(float)(lr * T.lr_factor);      // the product in double, rounded to fp32 once
    a.momentum = momentum;
    a.wd = T.weight_decay;
    a.first = first;
    a.zero = zero;
    float* __restrict__ P = T.d_p;
    float* __restrict__ G = T.d_g;
    float* __restrict__ B = T.d_buf;
    const int tid = threadIdx.x;

    if (T.form != DAFNE_SGD_CONV) {
        const int64_t base = (int64_t)ck.a * SGD_ELEMS;
        float* copy = T.form == DAFNE_SGD_F32 ? T.d_copy : nullptr;
        const float* addend = T.form == DAFNE_SGD_F32 ? T.d_addend : nullptr;
        for (int k = 0; k < SGD_ELEMS / SGD_THREADS; k++) {
            const int64_t i = base + k * SGD_THREADS + tid;
            if (i >= T.n) break;
            float buf = first ? 0.0f : B[i];
            const float pn = sgd_elem(P[i], G[i], buf, a);
            P[i] = pn;
            B[i] = buf;
            if (zero) G[i] = 0.0f;
            if (copy) copy[i] = addend ? pn + addend[i] : pn;
        }
        return;
    }

    const int taps = T.KH * T.KW;
    const int slab_f = 64 * taps;                               // fp32 of one (row, slab)
    const int K = T.Cin * taps;
    const int co0 = ck.a * SGD_ROWS;
    const int rows = min(SGD_ROWS, T.Cout - co0);
    const int slab = ck.b;
    // phase 1: the fp32 side, float4 by float4; the rounded new weights into LDS in the packed order (tap, channel in slab)
    const int v4_row = slab_f / 4;
    for (int i = tid; i < rows * v4_row; i += SGD_THREADS) {
        const int r = i / v4_row, v = i - r * v4_row;
        const int64_t off = ((int64_t)(co0 + r) * T.Cin + slab * 64) * taps + 4 * v;
        const float4 p4 = *reinterpret_cast<const float4*>(P + off);
        const float4 g4 = *reinterpret_cast<const float4*>(G + off);
        float4 b4 = first ? make_float4(0.f, 0.f, 0.f, 0.f) : *reinterpret_cast<const float4*>(B + off);
        float4 n4;
        n4.x = sgd_elem(p4.x, g4.x, b4.x, a);
        n4.y = sgd_elem(p4.y, g4.y, b4.y, a);
        n4.z = sgd_elem(p4.z, g4.z, b4.z, a);
        n4.w = sgd_elem(p4.w, g4.w, b4.w, a);
        *reinterpret_cast<float4*>(P + off) = n4;
        *reinterpret_cast<float4*>(B + off) = b4;
        if (zero) *reinterpret_cast<float4*>(G + off) = make_float4(0.f, 0.f, 0.f, 0.f);
        const float nv[4] = {n4.x, n4.y, n4.z, n4.w};
#pragma unroll
        for (int e = 0; e < 4; e++) {
            const int s = 4 * v + e;                            // OIHW inside the slab: channel * taps + tap
            const int c = s / taps, t = s - c * taps;
            lds[r * SGD_LDS_ROW + t * 64 + c] = bf16_rne(nv[e]);
        }
    }
    __syncthreads();
    // phase 2: 16-byte groups = 8 consecutive K columns of one row
    const int g_row = slab_f / 8;                               // groups per (row, slab)
    const int kg0 = slab * g_row;                               // first K group of this slab in the row
    uint4* plain = reinterpret_cast<uint4*>(T.d_plain);
    for (int i = tid; i < rows * g_row; i += SGD_THREADS) {     // plain form: groups of a row are contiguous
        const int r = i / g_row, q = i - r * g_row;
        const uint4 v = *reinterpret_cast<const uint4*>(&lds[r * SGD_LDS_ROW + q * 8]);
        plain[(int64_t)(T.row0 + co0 + r) * (K / 8) + kg0 + q] = v;
    }
    if (T.d_frag || T.d_wr || T.d_frag16) {
        uint4* frag = reinterpret_cast<uint4*>(T.d_frag);
        uint4* wr = reinterpret_cast<uint4*>(T.d_wr);
        uint4* frag16 = reinterpret_cast<uint4*>(T.d_frag16);
        for (int i = tid; i < rows * g_row; i += SGD_THREADS) { // fragment forms: the rows of one K group are contiguous
            const int q = i / rows, r = i - q * rows;
            const uint4 v = *reinterpret_cast<const uint4*>(&lds[r * SGD_LDS_ROW + q * 8]);
            const int row = T.row0 + co0 + r, kg = kg0 + q;     // absolute row, K group (K column / 8)
            const int64_t nt_w = row >> 5;                      // (row / 256) * 8 + (row % 256) / 32
            if (frag || wr) {
                // [nt][wave][K/16 steps][2 halves][32 rows][8]
                const int64_t o = ((nt_w * (K / 16) + (kg >> 1)) * 2 + (kg & 1)) * 32 + (row & 31);
                if (frag) frag[o] = v;
                if (wr) wr[o] = v;
            }
            if (frag16) {
                // [nt][wave][K/32][2 row halves][4 K quarters][16 rows][8]
                const int64_t o = (((nt_w * (K / 32) + (kg >> 2)) * 2 + ((row >> 4) & 1)) * 4 + (kg & 3)) * 16 + (row & 15);
                frag16[o] = v;
            }
        }
    }
}

inline int al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// DAFNE_OK, or the refusal of descriptor i with the message set
inline int validate(const dafne_sgd_tensor* t, int n_tensors) {
    if (!t || n_tensors <= 0) return dafne::fail(DAFNE_E_INVALID, "sgd: no tensors (tensors %p, n_tensors %d)", (const void*)t, n_tensors);
    for (int i = 0; i < n_tensors; i++) {
        const dafne_sgd_tensor& T = t[i];
        if (!T.d_p || !T.d_g || !T.d_buf) return dafne::fail(DAFNE_E_INVALID, "sgd: tensor %d: null d_p / d_g / d_buf", i);
        if (T.n <= 0 || T.n > 0x7fffffffll) return dafne::fail(DAFNE_E_INVALID, "sgd: tensor %d: n = %lld", i, (long long)T.n);
        if (T.form == DAFNE_SGD_NONE) continue;
        if (T.form == DAFNE_SGD_F32) {
            if (!T.d_copy) return dafne::fail(DAFNE_E_INVALID, "sgd: tensor %d: form F32 without d_copy", i);
            continue;
        }
        if (T.form != DAFNE_SGD_CONV) return dafne::fail(DAFNE_E_INVALID, "sgd: tensor %d: unknown form %d", i, T.form);
        if (!T.d_plain) return dafne::fail(DAFNE_E_INVALID, "sgd: tensor %d: form CONV without d_plain", i);
        if (T.Cout < 1 || T.Cin < 1 || T.KH < 1 || T.KW < 1 || T.row0 < 0 || T.rows < 1 || T.row0 > T.rows - T.Cout)
            return dafne::fail(DAFNE_E_INVALID, "sgd: tensor %d: Cout %d Cin %d %dx%d, rows %d..+%d of %d", i, T.Cout, T.Cin, T.KH, T.KW,
                               T.row0, T.Cout, T.rows);
        if (T.Cin % 64 != 0) return dafne::fail(DAFNE_E_UNSUPPORTED, "sgd: tensor %d: Cin %d is no multiple of 64 (pack_conv's slabs)", i, T.Cin);
        if ((int64_t)T.KH * T.KW > SGD_MAX_TAPS)
            return dafne::fail(DAFNE_E_UNSUPPORTED, "sgd: tensor %d: %dx%d taps, at most %d", i, T.KH, T.KW, SGD_MAX_TAPS);
        if ((int64_t)T.Cout * T.Cin * T.KH * T.KW != T.n)
            return dafne::fail(DAFNE_E_INVALID, "sgd: tensor %d: n = %lld is not Cout * Cin * KH * KW", i, (long long)T.n);
        if ((int64_t)T.rows * T.Cin * T.KH * T.KW > 0x7fffffffll)
            return dafne::fail(DAFNE_E_UNSUPPORTED, "sgd: tensor %d: packed matrix above 2^31 elements", i);
        if ((T.d_frag || T.d_frag16 || T.d_wr) && T.rows % 256 != 0)
            return dafne::fail(DAFNE_E_UNSUPPORTED, "sgd: tensor %d: fragment forms need a packed matrix of 256-row tiles, got %d rows", i, T.rows);
        if (!al16(T.d_p) || !al16(T.d_g) || !al16(T.d_buf) || !al16(T.d_plain) || !al16(T.d_frag) || !al16(T.d_frag16) || !al16(T.d_wr))
            return dafne::fail(DAFNE_E_INVALID, "sgd: tensor %d: form CONV needs 16-byte aligned pointers", i);
    }
    return DAFNE_OK;
}

inline int64_t chunks_of(const dafne_sgd_tensor& T) {
    if (T.form == DAFNE_SGD_CONV) return (int64_t)((T.Cout + SGD_ROWS - 1) / SGD_ROWS) * (T.Cin / 64);
    return (T.n + SGD_ELEMS - 1) / SGD_ELEMS;
}

inline int64_t count_chunks(const dafne_sgd_tensor* t, int n_tensors) {
    int64_t n = 0;
    for (int i = 0; i < n_tensors; i++) n += chunks_of(t[i]);
    return n;
}

}  // namespace dafne_sgd

extern "C" {
using dafne_sgd::Chunk;
using dafne_sgd::SGD_ROWS;
using dafne_sgd::SGD_THREADS;

int dafne_sgd_num_chunks(const dafne_sgd_tensor* tensors, int n_tensors) {
    if (dafne_sgd::validate(tensors, n_tensors) != DAFNE_OK) return -1;
    const int64_t n = dafne_sgd::count_chunks(tensors, n_tensors);
    if (n > 0x7fffffffll) {
        dafne::fail(DAFNE_E_UNSUPPORTED, "sgd: %lld chunks", (long long)n);
        return -1;
    }
    return (int)n;
}

size_t dafne_sgd_table_bytes(const dafne_sgd_tensor* tensors, int n_tensors) {
    const int n = dafne_sgd_num_chunks(tensors, n_tensors);
    return n < 0 ? 0 : (size_t)n_tensors * sizeof(dafne_sgd_tensor) + (size_t)n * sizeof(Chunk);
}

int dafne_sgd_table_build(const dafne_sgd_tensor* tensors, int n_tensors, void* h_table, size_t table_bytes) {
    const size_t need = dafne_sgd_table_bytes(tensors, n_tensors);
    if (need == 0) return DAFNE_E_INVALID;          // (message set by the validation)
    if (!h_table) return dafne::fail(DAFNE_E_INVALID, "sgd: null h_table");
    if (table_bytes < need) return dafne::fail(DAFNE_E_WORKSPACE, "sgd: table of %zu bytes, %zu needed", table_bytes, need);
    memcpy(h_table, tensors, (size_t)n_tensors * sizeof(dafne_sgd_tensor));
    Chunk* c = reinterpret_cast<Chunk*>(static_cast<char*>(h_table) + (size_t)n_tensors * sizeof(dafne_sgd_tensor));
    // the convolution chunks first: they carry nearly all the bytes and start on an empty chip
    for (int pass = 0; pass < 2; pass++)
        for (int i = 0; i < n_tensors; i++) {
            const dafne_sgd_tensor& T = tensors[i];
            if ((T.form == DAFNE_SGD_CONV) != (pass == 0)) continue;
            if (pass == 0) {
                for (int rb = 0; rb < (T.Cout + SGD_ROWS - 1) / SGD_ROWS; rb++)
                    for (int s = 0; s < T.Cin / 64; s++) *c++ = Chunk{i, rb, s, 0};
            } else {
                for (int64_t k = 0; k < dafne_sgd::chunks_of(T); k++) *c++ = Chunk{i, (int32_t)k, 0, 0};
            }
        }
    return DAFNE_OK;
}

int dafne_sgd_step_hip(const dafne_sgd_tensor* tensors, int n_tensors, const void* d_table, size_t table_bytes, double lr,
                       double momentum, int first_step, int zero_grad, void* stream) {
    const size_t need = dafne_sgd_table_bytes(tensors, n_tensors);
    if (need == 0) return DAFNE_E_INVALID;          // (message set by the validation)
    if (!d_table) return dafne::fail(DAFNE_E_INVALID, "sgd: null d_table");
    if (!dafne_sgd::al16(d_table)) return dafne::fail(DAFNE_E_INVALID, "sgd: d_table is not 16-byte aligned");
    if (table_bytes < need) return dafne::fail(DAFNE_E_WORKSPACE, "sgd: table of %zu bytes, %zu needed", table_bytes, need);
    if (!(lr >= 0.0) || !(momentum >= 0.0)) return dafne::fail(DAFNE_E_INVALID, "sgd: lr %g, momentum %g", lr, momentum);
    const int n_chunks = (int)dafne_sgd::count_chunks(tensors, n_tensors);
    const dafne_sgd_tensor* dt = static_cast<const dafne_sgd_tensor*>(d_table);
    const Chunk* dc = reinterpret_cast<const Chunk*>(dt + n_tensors);
    hipLaunchKernelGGL(dafne_sgd::sgd_step_kernel, dim3(n_chunks), dim3(SGD_THREADS), 0, static_cast<hipStream_t>(stream), dt, dc, lr,
                       (float)momentum, first_step ? 1 : 0, zero_grad ? 1 : 0);
    return dafne::check_launch("sgd_step_kernel");
}

}  // extern "C"
