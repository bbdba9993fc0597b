// Decode / threshold / per-level top-k / canonical corner order / gather for gfx950.
//
// Replaces the chain of small torch ops in DAFNeOutputs.forward_for_single_feature_map
// (dafne/modeling/dafne/dafne_outputs.py:792-905, stride multiply :771-772), the
// centre-to-corner epilogue of DAFNeHead.forward (dafne/modeling/dafne/dafne.py:405-411),
// compute_locations (dafne.py:37-44), sort_quadrilateral (dafne/utils/sort_corners.py:26-92)
// and detector_postprocess + OneStageDetector._postprocess
// (dafne/modeling/one_stage_detector.py:79-98).
//
// HBM-bound integer/selection work, no host round trips (the reference syncs with
// .item() per image and level, :851):
//   decode_hist      every (image, level, location, class): score, threshold test,
//                    11-bit histogram of the candidates' score keys (LDS-private)
//   decode_pick      per (image, level): histogram bin that holds the k-th best score
//   decode_collect   candidates above that bin -> selected list S, inside it -> E
//                    (wave-aggregated appends)
//   decode_finalize  per (image, level): exact radix select inside E (score, then
//                    lowest flat index among equal scores), bitonic sort of S by flat
//                    index (= the reference's nonzero() order), box decode, corner sort
//   gather_kernel    kept rows -> final detection rows (+ rescale / clip / drop empty)
//
// fp32 arithmetic is written in the reference's operation order and this file is
// compiled with -ffp-contract=off.
#include "common.h"
#include "sort_quad.h"
#include <string.h>

namespace {

typedef unsigned long long u64;
constexpr int kMaxLevels = 8;
constexpr int kBins = 2048;
constexpr int kChunk = 4096;     // elements per decode_hist / decode_collect block
constexpr int kMaxTopk = 4096;

struct LevelDev {
    const float* logits;
    const float* delta;
    const float* center;
    const float* ctrness;
    int logits_ps, delta_ps, center_ps, ctrness_ps;
    int H, W, stride;
    float scale;
    int chunk0;      // first chunk id of this level
    int n_elem;      // H*W*C
    size_t e_off;    // offset of this level's E list (entries) inside one image's E area
};

struct DecodeDev {
    LevelDev lv[kMaxLevels];
    int n_images, n_levels, C, topk, twc, sortc, m_cap;
    int no_center, no_ctr;   // DAFNE_DECODE_NO_CENTER / _NO_CTRNESS
    float thresh;
    unsigned key_lo;   // score bits are keyed as (bits - key_lo)
    int shift;         // histogram bin = key >> shift
    int n_chunks;      // per image
    int kp;            // topk rounded up to a power of two (sort width)
    size_t e_per_image;
    // workspace
    unsigned* hist;    // [N][L][kBins]
    int* meta;         // [N][L][4]: b1, k1, ncand, nsel
    unsigned* s_cnt;   // [N][L]
    unsigned* e_cnt;   // [N][L]
    u64* S;            // [N][L][kp]
    u64* E;            // [N][e_per_image]
};

__device__ __forceinline__ float sigmoidf_ref(float x) { return 1.0f / (1.0f + expf(-x)); }

// score + candidate test for element (loc, c) of one level (dafne_outputs.py:804-829)
__device__ __forceinline__ bool score_of(const DecodeDev& P, const LevelDev& L, int img, int loc, int c,
                                         float& score, float& ctr_out) {
    const size_t px = (size_t)img * L.H * L.W + loc;
    float cls = sigmoidf_ref(L.logits[px * L.logits_ps + c]);
    if (P.no_ctr) {          // CENTERNESS none (dafne_outputs.py:810-829): no sqrt, no centerness factor, THRESH_WITH_CTR moot
        ctr_out = 1.0f;
        score = cls;
        return cls > P.thresh;
    }
    float ctr = sigmoidf_ref(L.ctrness[px * L.ctrness_ps]);
    ctr_out = ctr;
    bool cand;
    if (P.twc) {
        score = sqrtf(cls * ctr);
        cand = score > P.thresh;
    } else {
        cand = cls > P.thresh;
        score = sqrtf(cls * ctr);
    }
    return cand;
}

__device__ __forceinline__ unsigned key_of(const DecodeDev& P, float score) {
    unsigned b = __float_as_uint(score);
    return b > P.key_lo ? b - P.key_lo : 0u;   // scores are positive; clamp is for safety
}

__device__ __forceinline__ int find_level(const DecodeDev& P, int chunk) {
    int l = 0;
#pragma unroll
    for (int k = 1; k < kMaxLevels; k++)
        if (k < P.n_levels && chunk >= P.lv[k].chunk0) l = k;
    return l;
}

// ----------------------------------------------------------------- decode_hist
__global__ void __launch_bounds__(256) decode_hist_kernel(DecodeDev P) {
    __shared__ unsigned h[kBins];
    const int img = blockIdx.y;
    const int lvl = find_level(P, blockIdx.x);
    const LevelDev& L = P.lv[lvl];
    for (int k = threadIdx.x; k < kBins; k += 256) h[k] = 0;
    __syncthreads();
    const int e0 = (blockIdx.x - L.chunk0) * kChunk;
    for (int e = e0 + threadIdx.x; e < min(e0 + kChunk, L.n_elem); e += 256) {
        int loc = e / P.C, c = e - loc * P.C;
        float s, ctr;
        if (score_of(P, L, img, loc, c, s, ctr)) {
            unsigned bin = min(key_of(P, s) >> P.shift, (unsigned)(kBins - 1));
            atomicAdd(&h[bin], 1u);
        }
    }
    __syncthreads();
    unsigned* g = P.hist + ((size_t)img * P.n_levels + lvl) * kBins;
    for (int k = threadIdx.x; k < kBins; k += 256)
        if (h[k]) atomicAdd(&g[k], h[k]);
}

// ----------------------------------------------------------------- decode_pick
__global__ void __launch_bounds__(64) decode_pick_kernel(DecodeDev P) {
    const int img = blockIdx.y, lvl = blockIdx.x, lane = threadIdx.x;
    const unsigned* g = P.hist + ((size_t)img * P.n_levels + lvl) * kBins;
    // lane owns bins [32*lane, 32*lane+32); suffix sums from the top
    unsigned mine = 0;
    for (int k = 0; k < 32; k++) mine += g[lane * 32 + k];
    unsigned suf = mine;   // inclusive suffix: bins >= 32*lane
    for (int o = 1; o < 64; o <<= 1) {
        unsigned v = __shfl_down(suf, o, 64);
        if (lane + o < 64) suf += v;
    }
    const unsigned total = __shfl(suf, 0, 64);
    int* meta = P.meta + ((size_t)img * P.n_levels + lvl) * 4;
    if (total <= (unsigned)P.topk) {
        if (lane == 0) {
            meta[0] = -1;
            meta[1] = 0;
            meta[2] = (int)total;
            meta[3] = (int)total;
        }
        return;
    }
    // the crossing lane: above = suf - mine < k <= suf
    const unsigned above = suf - mine;
    if (above < (unsigned)P.topk && suf >= (unsigned)P.topk) {
        unsigned acc = above;
        int b1 = lane * 32;
        for (int k = 31; k >= 0; k--) {
            unsigned hk = g[lane * 32 + k];
            if (acc + hk >= (unsigned)P.topk) {
                b1 = lane * 32 + k;
                break;
            }
            acc += hk;
        }
        meta[0] = b1;
        meta[1] = P.topk - (int)acc;   // how many to take from bin b1
        meta[2] = (int)total;
        meta[3] = P.topk;
    }
}

// -------------------------------------------------------------- decode_collect
__device__ __forceinline__ void wave_append(bool pred, u64 entry, u64* list, unsigned* counter,
                                            unsigned cap) {
    u64 b = __ballot(pred);
    if (!b) return;
    const int lane = threadIdx.x & 63;
    unsigned base = 0;
    const int leader = __ffsll((long long)b) - 1;
    if (lane == leader) base = atomicAdd(counter, (unsigned)__popcll(b));
    base = __shfl(base, leader, 64);
    if (pred) {
        unsigned slot = base + (unsigned)__popcll(b & ((1ull << lane) - 1ull));
        if (slot < cap) list[slot] = entry;
    }
}

__global__ void __launch_bounds__(256) decode_collect_kernel(DecodeDev P) {
    const int img = blockIdx.y;
    const int lvl = find_level(P, blockIdx.x);
    const LevelDev& L = P.lv[lvl];
    const size_t il = (size_t)img * P.n_levels + lvl;
    const int b1 = P.meta[il * 4 + 0];
    u64* S = P.S + il * P.kp;
    u64* E = P.E + (size_t)img * P.e_per_image + L.e_off;
    const int e0 = (blockIdx.x - L.chunk0) * kChunk;
    const int e1 = min(e0 + kChunk, L.n_elem);
    for (int eb = e0; eb < e1; eb += 256) {   // uniform trip count: ballots need whole waves
        int e = eb + threadIdx.x;
        bool live = e < e1, cand = false;
        float s = 0.f, ctr;
        if (live) {
            int loc = e / P.C, c = e - loc * P.C;
            cand = score_of(P, L, img, loc, c, s, ctr);
        }
        int bin = cand ? (int)min(key_of(P, s) >> P.shift, (unsigned)(kBins - 1)) : -2;
        u64 entry = ((u64)__float_as_uint(s) << 32) | (unsigned)e;
        wave_append(cand && bin > b1, entry, S, P.s_cnt + il, (unsigned)P.kp);
        wave_append(cand && bin == b1, entry, E, P.e_cnt + il, (unsigned)L.n_elem);
    }
}

// ------------------------------------------------------- sort_quadrilateral
// the device function lives in sort_quad.h (targets_kernels.h sorts the predicted corners of positives with it)
using dafne::sort_quad;

__global__ void __launch_bounds__(256) sort_quad_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                        long long n) {
    long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float q[8];
#pragma unroll
    for (int k = 0; k < 8; k++) q[k] = in[i * 8 + k];
    sort_quad(q);
#pragma unroll
    for (int k = 0; k < 8; k++) out[i * 8 + k] = q[k];
}

// ------------------------------------------------------------- decode_finalize
constexpr int kFinThreads = 1024;

// one radix step inside the workgroup: histogram `nbits` bits of f(entry) at
// `shift` over entries that pass `match`, then walk the bins (from the top when
// `descending`) until `need` is covered.  Returns the chosen bin and updates need.
template <typename KeyFn, typename MatchFn>
__device__ int radix_step(const u64* E, int n, int nbits, unsigned* h, KeyFn key, MatchFn match,
                          bool descending, int& need) {
    const int nb = 1 << nbits;
    for (int k = threadIdx.x; k < nb; k += kFinThreads) h[k] = 0;
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += kFinThreads) {
        u64 en = E[i];
        if (match(en)) atomicAdd(&h[key(en) & (nb - 1)], 1u);
    }
    __syncthreads();
    __shared__ int s_bin, s_need;
    // the bin in which the running count (from the top when `descending`) reaches `need`: wave 0, lane l owns `per`
    // consecutive bins in walk order; a wave scan finds the lane that holds the crossing, which then walks its own bins.
    // (Round 3 walked all 2048 bins on ONE thread -- dependent LDS reads, ~60 us per step, four steps per (image, level):
    // the whole 245 us of this kernel.)
    if (threadIdx.x < 64) {
        const int lane = threadIdx.x;
        const int per = nb >= 64 ? nb / 64 : 1;
        const int t0 = lane * per;                               // first walk position of this lane
        int mine = 0;
        if (t0 < nb)
            for (int t = 0; t < per; t++) mine += (int)h[descending ? nb - 1 - (t0 + t) : t0 + t];
        int incl = mine;                                         // inclusive prefix over lanes in walk order
        for (int o = 1; o < 64; o <<= 1) {
            const int v = __shfl_up(incl, o, 64);
            if (lane >= o) incl += v;
        }
        const int before = incl - mine;
        const int total = __shfl(incl, 63, 64);
        if (need <= 0) {                                         // (not reached by the callers) the serial walk stops at once
            if (lane == 0) { s_bin = descending ? nb - 1 : 0; s_need = need; }
        } else if (total < need) {                               // never reached: the walk's defaults
            if (lane == 0) { s_bin = descending ? nb - 1 : 0; s_need = need - total; }
        } else if (before < need && incl >= need) {              // exactly one lane (need >= 1)
            int acc = before, bin = descending ? nb - 1 - t0 : t0;
            for (int t = 0; t < per; t++) {
                const int b = descending ? nb - 1 - (t0 + t) : t0 + t;
                const int hv = (int)h[b];
                if (acc + hv >= need) { bin = b; break; }
                acc += hv;
            }
            s_bin = bin;
            s_need = need - acc;
        }
    }
    __syncthreads();
    need = s_need;
    int r = s_bin;
    __syncthreads();
    return r;
}

__global__ void __launch_bounds__(kFinThreads) decode_finalize_kernel(
    DecodeDev P, float* __restrict__ o_corners, float* __restrict__ o_scores, float* __restrict__ o_ctr,
    int* __restrict__ o_classes, float* __restrict__ o_locs, int* __restrict__ o_levels,
    float* __restrict__ o_hbox, int* __restrict__ o_counts) {
    const int img = blockIdx.y, lvl = blockIdx.x, tid = threadIdx.x;
    const LevelDev& L = P.lv[lvl];
    const size_t il = (size_t)img * P.n_levels + lvl;
    const int* meta = P.meta + il * 4;
    const int b1 = meta[0];
    const int nsel = meta[3];
    u64* S = P.S + il * P.kp;
    const u64* E = P.E + (size_t)img * P.e_per_image + L.e_off;

    __shared__ unsigned h[kBins];
    __shared__ u64 srt[kMaxTopk];
    __shared__ unsigned s_app;

    if (b1 >= 0) {
        // exact selection of k1 entries out of bin b1: largest scores first, equal
        // scores by smallest flat index (oracle/postprocess.py decode_level)
        const int n = (int)min(P.e_cnt[il], (unsigned)L.n_elem);
        int need = meta[1];
        unsigned prefix = (unsigned)b1;      // key >> bits_left so far
        int bits_left = P.shift;
        while (bits_left > 0) {
            const int nbits = min(11, bits_left);
            const int sh = bits_left - nbits;
            const unsigned pf = prefix;
            const int bl = bits_left;
            const unsigned lo = P.key_lo;
            auto keyf = [=](u64 en) { unsigned k = (unsigned)(en >> 32); k = k > lo ? k - lo : 0u; return k >> sh; };
            auto matchf = [=](u64 en) { unsigned k = (unsigned)(en >> 32); k = k > lo ? k - lo : 0u; return (k >> bl) == pf; };
            int bin = radix_step(E, n, nbits, h, keyf, matchf, true, need);
            prefix = (prefix << nbits) | (unsigned)bin;
            bits_left = sh;
        }
        const unsigned tkey = prefix;        // exact key of the k-th best score
        // ties at tkey: take the `need` smallest flat indices
        int ibits = 1;
        while ((1 << ibits) < L.n_elem) ibits++;
        unsigned iprefix = 0;
        int ileft = ibits;
        const unsigned lo = P.key_lo;
        while (ileft > 0) {
            const int nbits = min(11, ileft);
            const int sh = ileft - nbits;
            const unsigned pf = iprefix;
            const int bl = ileft;
            auto keyf = [=](u64 en) { return (unsigned)en >> sh; };
            auto matchf = [=](u64 en) {
                unsigned k = (unsigned)(en >> 32); k = k > lo ? k - lo : 0u;
                return k == tkey && (((unsigned)en) >> bl) == pf;
            };
            int bin = radix_step(E, n, nbits, h, keyf, matchf, false, need);
            iprefix = (iprefix << nbits) | (unsigned)bin;
            ileft = sh;
        }
        const unsigned icut = iprefix;       // ties with flat index <= icut are taken
        if (tid == 0) s_app = P.s_cnt[il];
        __syncthreads();
        for (int i0 = 0; i0 < n; i0 += kFinThreads) {
            int i = i0 + tid;
            bool take = false;
            u64 en = 0;
            if (i < n) {
                en = E[i];
                unsigned k = (unsigned)(en >> 32); k = k > lo ? k - lo : 0u;
                take = k > tkey || (k == tkey && (unsigned)en <= icut);
            }
            wave_append(take, en, S, &s_app, (unsigned)P.kp);
        }
        __syncthreads();
    }

    // sort the selected entries by flat index (location major, class minor)
    for (int i = tid; i < P.kp; i += kFinThreads) {
        u64 en = i < nsel ? S[i] : ~0ull;
        srt[i] = i < nsel ? ((en << 32) | (en >> 32)) : ~0ull;   // (flat, score bits)
    }
    __syncthreads();
    for (int k = 2; k <= P.kp; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < P.kp; i += kFinThreads) {
                int ixj = i ^ j;
                if (ixj > i) {
                    u64 a = srt[i], b = srt[ixj];
                    bool up = (i & k) == 0;
                    if ((a > b) == up) { srt[i] = b; srt[ixj] = a; }
                }
            }
            __syncthreads();
        }
    }

    int off = 0;
    for (int l2 = 0; l2 < lvl; l2++) off += P.meta[((size_t)img * P.n_levels + l2) * 4 + 3];
    if (lvl == 0 && tid == 0) {
        int tot = 0;
        for (int l2 = 0; l2 < P.n_levels; l2++) tot += P.meta[((size_t)img * P.n_levels + l2) * 4 + 3];
        o_counts[img] = tot;
    }
    const float fs = (float)L.stride;
    const float half = (float)(L.stride / 2);
    for (int r = tid; r < nsel; r += kFinThreads) {
        const u64 en = srt[r];
        const int flat = (int)(en >> 32);
        const float score = __uint_as_float((unsigned)en);
        const int loc = flat / P.C, c = flat - loc * P.C;
        const int y = loc / L.W, x = loc - y * L.W;
        const float lx = (float)(x * L.stride) + half;   // dafne.py:37-44
        const float ly = (float)(y * L.stride) + half;
        const size_t px = (size_t)img * L.H * L.W + loc;
        const float* dl = L.delta + px * L.delta_ps;
        float cx = 0.f, cy = 0.f;
        if (!P.no_center) {
            const float* ce = L.center + px * L.center_ps;
            cx = ce[0]; cy = ce[1];
        }
        float q[8];
#pragma unroll
        for (int j = 0; j < 8; j++) {
            // dafne.py:403  center.repeat + delta; direct / offset / iterative heads (no center): the regression itself
            float reg = P.no_center ? dl[j] : ((j & 1) ? cy : cx) + dl[j];
            reg = reg * L.scale;                         // dafne.py:406  Scale
            reg = reg * fs;                              // dafne_outputs.py:771-772
            q[j] = ((j & 1) ? ly : lx) + reg;            // dafne_outputs.py:861-873
        }
        if (P.sortc) sort_quad(q);
        const size_t row = (size_t)img * P.m_cap + off + r;
        if (off + r < P.m_cap) {
#pragma unroll
            for (int j = 0; j < 8; j++) o_corners[row * 8 + j] = q[j];
            o_scores[row] = score;
            o_ctr[row] = P.no_ctr ? 1.0f : sigmoidf_ref(L.ctrness[px * L.ctrness_ps]);
            o_classes[row] = c;
            o_locs[row * 2 + 0] = lx;
            o_locs[row * 2 + 1] = ly;
            o_levels[row] = lvl;
            o_hbox[row * 4 + 0] = fminf(fminf(q[0], q[2]), fminf(q[4], q[6]));
            o_hbox[row * 4 + 1] = fminf(fminf(q[1], q[3]), fminf(q[5], q[7]));
            o_hbox[row * 4 + 2] = fmaxf(fmaxf(q[0], q[2]), fmaxf(q[4], q[6]));
            o_hbox[row * 4 + 3] = fmaxf(fmaxf(q[1], q[3]), fmaxf(q[5], q[7]));
        }
    }
}

// -------------------------------------------------------------------- gather
__global__ void __launch_bounds__(1024) gather_kernel(
    const float* __restrict__ corners, const float* __restrict__ scores, const float* __restrict__ ctr,
    const int* __restrict__ classes, const float* __restrict__ locs, const int* __restrict__ levels,
    const float* __restrict__ hbox, const long long* __restrict__ keep, const int* __restrict__ num_keep,
    const float* __restrict__ sizes, int do_post, int m_cap, int k_cap, float* __restrict__ out,
    int* __restrict__ out_counts) {
    const int img = blockIdx.x, tid = threadIdx.x;
    const int nk = min(num_keep[img], m_cap);
    float sx = 1.f, sy = 1.f, cxs = 1.f, cys = 1.f, oh = 0.f, ow = 0.f;
    if (do_post) {
        const float* sz = sizes + img * 6;   // net_h, net_w, out_h, out_w, orig_h, orig_w
        oh = sz[2]; ow = sz[3];
        sx = (float)((double)sz[3] / (double)sz[1]);   // python float division, then fp32 multiply
        sy = (float)((double)sz[2] / (double)sz[0]);
        if (do_post >= 2) {   // OneStageDetector._postprocess (skipped by the TTA path)
            cxs = (float)((double)sz[3] / (double)sz[5]);
            cys = (float)((double)sz[2] / (double)sz[4]);
        }
    }
    __shared__ int wsum[16];
    __shared__ int s_base;
    if (tid == 0) s_base = 0;
    __syncthreads();
    for (int r0 = 0; r0 < nk; r0 += 1024) {
        const int r = r0 + tid;
        bool ok = r < nk;
        size_t src = 0;
        float hb[4] = {0, 0, 0, 0};
        if (ok) {
            src = (size_t)img * m_cap + (size_t)keep[(size_t)img * m_cap + r];
#pragma unroll
            for (int j = 0; j < 4; j++) hb[j] = hbox[src * 4 + j];
            if (do_post) {
                hb[0] *= sx; hb[2] *= sx; hb[1] *= sy; hb[3] *= sy;          // Boxes.scale
                hb[0] = fminf(fmaxf(hb[0], 0.f), ow); hb[2] = fminf(fmaxf(hb[2], 0.f), ow);   // Boxes.clip
                hb[1] = fminf(fmaxf(hb[1], 0.f), oh); hb[3] = fminf(fmaxf(hb[3], 0.f), oh);
                ok = (hb[2] - hb[0]) > 0.f && (hb[3] - hb[1]) > 0.f;         // Boxes.nonempty
            }
        }
        // ordered compaction: wave ballot + per-wave offsets
        u64 b = __ballot(ok);
        const int lane = tid & 63, wv = tid >> 6;
        if (lane == 0) wsum[wv] = __popcll(b);
        __syncthreads();
        int woff = 0, tot = 0;
        for (int k = 0; k < 16; k++) {
            if (k < wv) woff += wsum[k];
            tot += wsum[k];
        }
        const int base = s_base;
        if (ok) {
            const int o = base + woff + __popcll(b & ((1ull << lane) - 1ull));
            if (o < k_cap) {
                float* d = out + ((size_t)img * k_cap + o) * DAFNE_DET_ROW;
#pragma unroll
                for (int j = 0; j < 8; j++) d[j] = corners[src * 8 + j] * ((j & 1) ? cys : cxs);
                d[8] = scores[src];
                d[9] = ctr[src];
                d[10] = (float)classes[src];
                d[11] = (float)levels[src];
                d[12] = hb[0]; d[13] = hb[1]; d[14] = hb[2]; d[15] = hb[3];
                d[16] = locs[src * 2 + 0] * cxs;
                d[17] = locs[src * 2 + 1] * cys;
            }
        }
        __syncthreads();
        if (tid == 0) s_base = base + tot;
        __syncthreads();
    }
    if (tid == 0) out_counts[img] = s_base;
}

int setup(DecodeDev& D, const dafne_decode_params* prm, const dafne_level_desc* levels, void* ws,
          size_t* need_out) {
    if (!prm || !levels) return dafne::fail(DAFNE_E_INVALID, "decode: null params");
    if (prm->n_levels < 1 || prm->n_levels > kMaxLevels) return dafne::fail(DAFNE_E_UNSUPPORTED, "decode: n_levels %d", prm->n_levels);
    if (prm->n_images < 1 || prm->n_classes < 1) return dafne::fail(DAFNE_E_INVALID, "decode: bad sizes");
    if (prm->pre_nms_topk < 1 || prm->pre_nms_topk > kMaxTopk) return dafne::fail(DAFNE_E_UNSUPPORTED, "decode: pre_nms_topk %d not in [1,%d]", prm->pre_nms_topk, kMaxTopk);
    if (prm->m_cap < prm->n_levels * prm->pre_nms_topk) return dafne::fail(DAFNE_E_INVALID, "decode: m_cap too small");
    D.n_images = prm->n_images; D.n_levels = prm->n_levels; D.C = prm->n_classes;
    D.topk = prm->pre_nms_topk; D.twc = prm->thresh_with_ctr; D.sortc = prm->sort_corners;
    D.m_cap = prm->m_cap; D.thresh = prm->pre_nms_thresh;
    if (prm->flags & ~(DAFNE_DECODE_NO_CENTER | DAFNE_DECODE_NO_CTRNESS))
        return dafne::fail(DAFNE_E_INVALID, "decode: unknown flags 0x%x", (unsigned)prm->flags);
    D.no_center = (prm->flags & DAFNE_DECODE_NO_CENTER) != 0;
    D.no_ctr = (prm->flags & DAFNE_DECODE_NO_CTRNESS) != 0;
    // key = bits - key_lo, top bin index < 2048.  THRESH_WITH_CTR: the ranked score IS the thresholded one, so
    // scores lie in (max(thresh,0), 1] and the key range starts at the threshold.  Otherwise the candidate test is
    // cls > thresh while the ranked score is sqrt(cls * ctr), anywhere in (0, 1] (dafne_outputs.py:812-829): the
    // key range must start at 0, or every score below the threshold would collapse into one key and top-k would
    // pick among them by flat index instead of by score.
    union { float f; unsigned u; } t, one;
    // (without centerness the ranked score is the thresholded sigmoid(cls): the key range starts at the threshold too)
    t.f = ((prm->thresh_with_ctr || D.no_ctr) && prm->pre_nms_thresh > 0.f) ? prm->pre_nms_thresh : 0.f;
    one.f = 1.0f;
    D.key_lo = t.u < one.u ? t.u : 0u;
    unsigned range = one.u - D.key_lo;
    D.shift = 0;
    while ((range >> D.shift) >= (unsigned)kBins) D.shift++;
    D.kp = 2;
    while (D.kp < D.topk) D.kp <<= 1;
    int chunk = 0;
    size_t eoff = 0;
    for (int l = 0; l < D.n_levels; l++) {
        const dafne_level_desc& s = levels[l];
        LevelDev& L = D.lv[l];
        L.logits = s.d_logits; L.delta = s.d_delta; L.center = s.d_center; L.ctrness = s.d_ctrness;
        L.logits_ps = s.logits_ps; L.delta_ps = s.delta_ps; L.center_ps = s.center_ps; L.ctrness_ps = s.ctrness_ps;
        L.H = s.H; L.W = s.W; L.stride = s.stride; L.scale = s.scale;
        if (s.H < 1 || s.W < 1 || (long long)s.H * s.W * D.C > 0x7fffffffLL) return dafne::fail(DAFNE_E_INVALID, "decode: level %d size", l);
        L.n_elem = s.H * s.W * D.C;
        L.chunk0 = chunk;
        chunk += (L.n_elem + kChunk - 1) / kChunk;
        L.e_off = eoff;
        eoff += (size_t)L.n_elem;
    }
    D.n_chunks = chunk;
    D.e_per_image = eoff;
    dafne::WsCarver c(ws);
    const size_t NL = (size_t)D.n_images * D.n_levels;
    D.hist = c.take<unsigned>(NL * kBins);
    D.s_cnt = c.take<unsigned>(NL);
    D.e_cnt = c.take<unsigned>(NL);      // hist, s_cnt, e_cnt are zeroed per call (contiguous)
    D.meta = c.take<int>(NL * 4);
    D.S = c.take<u64>(NL * D.kp);
    D.E = c.take<u64>((size_t)D.n_images * D.e_per_image);
    *need_out = dafne::align_up(c.off, 256);
    return DAFNE_OK;
}

}  // namespace

extern "C" {

size_t dafne_decode_workspace_bytes(const dafne_decode_params* prm, const dafne_level_desc* levels) {
    DecodeDev D;
    size_t need = 0;
    if (setup(D, prm, levels, nullptr, &need)) return 0;
    return need;
}

int dafne_decode_levels_hip(const dafne_decode_params* prm, const dafne_level_desc* levels,
                            float* d_corners, float* d_scores, float* d_ctr, int32_t* d_classes,
                            float* d_locs, int32_t* d_levels, float* d_hbox, int32_t* d_counts,
                            void* d_ws, size_t ws_bytes, void* stream) {
    DecodeDev D;
    size_t need = 0;
    int rc = setup(D, prm, levels, d_ws, &need);
    if (rc) return rc;
    if (!d_ws || ws_bytes < need) return dafne::fail(DAFNE_E_WORKSPACE, "decode: workspace %zu < %zu", ws_bytes, need);
    if (!d_corners || !d_scores || !d_ctr || !d_classes || !d_locs || !d_levels || !d_hbox || !d_counts)
        return dafne::fail(DAFNE_E_INVALID, "decode: null output");
    for (int l = 0; l < D.n_levels; l++)
        if (!D.lv[l].logits || !D.lv[l].delta || (!D.no_center && !D.lv[l].center) || (!D.no_ctr && !D.lv[l].ctrness))
            return dafne::fail(DAFNE_E_INVALID, "decode: null input at level %d", l);
    hipStream_t st = (hipStream_t)stream;
    size_t zbytes = (size_t)((char*)(D.e_cnt + (size_t)D.n_images * D.n_levels) - (char*)D.hist);
    DAFNE_HIP_TRY(hipMemsetAsync(D.hist, 0, zbytes, st));
    hipLaunchKernelGGL(decode_hist_kernel, dim3(D.n_chunks, D.n_images), dim3(256), 0, st, D);
    if ((rc = dafne::check_launch("decode_hist"))) return rc;
    hipLaunchKernelGGL(decode_pick_kernel, dim3(D.n_levels, D.n_images), dim3(64), 0, st, D);
    if ((rc = dafne::check_launch("decode_pick"))) return rc;
    hipLaunchKernelGGL(decode_collect_kernel, dim3(D.n_chunks, D.n_images), dim3(256), 0, st, D);
    if ((rc = dafne::check_launch("decode_collect"))) return rc;
    hipLaunchKernelGGL(decode_finalize_kernel, dim3(D.n_levels, D.n_images), dim3(kFinThreads), 0, st, D,
                       d_corners, d_scores, d_ctr, d_classes, d_locs, d_levels, d_hbox, d_counts);
    return dafne::check_launch("decode_finalize");
}

int dafne_sort_quadrilateral_hip(const float* d_in, float* d_out, int64_t n, void* stream) {
    if (n < 0 || (n > 0 && (!d_in || !d_out))) return dafne::fail(DAFNE_E_INVALID, "sort_quadrilateral: bad args");
    if (n == 0) return DAFNE_OK;
    hipLaunchKernelGGL(sort_quad_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       d_in, d_out, (long long)n);
    return dafne::check_launch("sort_quadrilateral");
}

int dafne_gather_detections_hip(const float* d_corners, const float* d_scores, const float* d_ctr,
                                const int32_t* d_classes, const float* d_locs,
                                const int32_t* d_levels, const float* d_hbox,
                                const int64_t* d_keep, const int32_t* d_num_keep,
                                const float* d_sizes, int do_postprocess, int n_images, int m_cap,
                                int k_cap, float* d_out, int32_t* d_out_counts, void* stream) {
    if (n_images < 1 || m_cap < 0 || k_cap < 1 || !d_corners || !d_scores || !d_ctr || !d_classes || !d_locs ||
        !d_levels || !d_hbox || !d_keep || !d_num_keep || !d_out || !d_out_counts ||
        (do_postprocess && !d_sizes))
        return dafne::fail(DAFNE_E_INVALID, "gather: bad args");
    hipLaunchKernelGGL(gather_kernel, dim3(n_images), dim3(1024), 0, (hipStream_t)stream, d_corners, d_scores,
                       d_ctr, d_classes, d_locs, d_levels, d_hbox, reinterpret_cast<const long long*>(d_keep),
                       d_num_keep, d_sizes, do_postprocess, m_cap, k_cap, d_out, d_out_counts);
    return dafne::check_launch("gather");
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------- TTA merge candidates
// The merge input of OneStageRCNNWithTTA (dafne/modeling/tta.py:237-262, _invert_and_concat_fast here) for many images at
// once: every view's packed rows (detect_packed(do_postprocess=False), [k_cap, DET_ROW] + a device count) go back through
// the inverse of the view's transforms -- un-flip (w - x), then (x * r1) * r2 with the float32 ratios, the float32
// operations in that order -- and land in its image's Candidates rows, views in slot order, each view's rows in their own
// order.  A view's offset is the sum of the (capped) counts of the image's earlier slots: no atomic decides a position.
// d_overflow[image] = 1 when a view of the image reports more rows than k_cap (rows_to_instances raises there).
namespace {

__global__ void __launch_bounds__(256) tta_candidates_kernel(
    const dafne_tta_view* __restrict__ views, const int* __restrict__ tile_beg, int k_cap, int m_cap,
    float* __restrict__ corners, float* __restrict__ scores, float* __restrict__ ctr, int* __restrict__ classes,
    float* __restrict__ locs, int* __restrict__ levels, float* __restrict__ hbox, int* __restrict__ counts,
    int* __restrict__ overflow) {
    const int img = blockIdx.x, j = blockIdx.y;
    const int beg = tile_beg[img], nv = tile_beg[img + 1] - beg;
    __shared__ int s_off;
    if (j == 0 && threadIdx.x == 0) {           // the image's totals: capped row count + overflow flag
        int tot = 0, ovf = 0;
        for (int k = 0; k < nv; k++) {
            const int c = *views[beg + k].d_count;
            ovf |= (c > k_cap || c < 0);
            tot += c < 0 ? 0 : (c > k_cap ? k_cap : c);
        }
        counts[img] = tot;
        overflow[img] = ovf;
    }
    if (j >= nv) return;
    const dafne_tta_view& d = views[beg + j];
    if (threadIdx.x == 0) {
        int off = 0;
        for (int k = 0; k < j; k++) {
            const int c = *views[beg + k].d_count;
            off += c < 0 ? 0 : (c > k_cap ? k_cap : c);
        }
        s_off = off;
    }
    __syncthreads();
    int n = *d.d_count;
    n = n < 0 ? 0 : (n > k_cap ? k_cap : n);
    const size_t base = (size_t)img * m_cap + s_off;
    const float fw = d.width, fh = d.height;
    const float rx1 = d.rx1, ry1 = d.ry1, rx2 = d.rx2, ry2 = d.ry2;
    for (int r = threadIdx.x; r < n; r += blockDim.x) {
        const float* src = d.d_rows + (size_t)r * DAFNE_DET_ROW;
        const size_t o = base + r;
        float lo_x = 0.f, hi_x = 0.f, lo_y = 0.f, hi_y = 0.f;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            float x = src[2 * k], y = src[2 * k + 1];
            if (d.flip_x) x = fw - x;
            if (d.flip_y) y = fh - y;
            x = x * rx1;
            x = x * rx2;
            y = y * ry1;
            y = y * ry2;
            corners[o * 8 + 2 * k] = x;
            corners[o * 8 + 2 * k + 1] = y;
            lo_x = k ? fminf(lo_x, x) : x;
            hi_x = k ? fmaxf(hi_x, x) : x;
            lo_y = k ? fminf(lo_y, y) : y;
            hi_y = k ? fmaxf(hi_y, y) : y;
        }
        scores[o] = src[8];
        ctr[o] = src[9];
        classes[o] = (int)src[10];
        levels[o] = (int)src[11];
        locs[o * 2] = src[16];
        locs[o * 2 + 1] = src[17];
        hbox[o * 4] = lo_x;
        hbox[o * 4 + 1] = lo_y;
        hbox[o * 4 + 2] = hi_x;
        hbox[o * 4 + 3] = hi_y;
    }
}

}  // namespace

extern "C" {

size_t dafne_tta_candidates_workspace_bytes(int n_views, int n_images) {
    if (n_views < 1 || n_images < 1) return 0;
    return dafne::align_up(sizeof(dafne_tta_view) * (size_t)n_views, 256) + dafne::align_up(sizeof(int) * ((size_t)n_images + 1), 256);
}

int dafne_tta_candidates_hip(const dafne_tta_view* views, int n_views, int n_images, int k_cap, int m_cap, float* d_corners,
                             float* d_scores, float* d_ctr, int32_t* d_classes, float* d_locs, int32_t* d_levels,
                             float* d_hbox, int32_t* d_counts, int32_t* d_overflow, void* d_ws, size_t ws_bytes, void* stream) {
    if (!views || n_views < 1 || n_images < 1 || k_cap < 1 || m_cap < 1 || !d_corners || !d_scores || !d_ctr || !d_classes ||
        !d_locs || !d_levels || !d_hbox || !d_counts || !d_overflow || !d_ws)
        return dafne::fail(DAFNE_E_INVALID, "tta_candidates: bad args (n_views %d, n_images %d, k_cap %d, m_cap %d)", n_views,
                           n_images, k_cap, m_cap);
    if (m_cap > 65536) return dafne::fail(DAFNE_E_UNSUPPORTED, "tta_candidates: m_cap %d above the NMS limit 65536", m_cap);
    const size_t need = dafne_tta_candidates_workspace_bytes(n_views, n_images);
    if (ws_bytes < need) return dafne::fail(DAFNE_E_WORKSPACE, "tta_candidates: workspace %zu < %zu", ws_bytes, need);
    // views grouped by image, in slot order (counting sort by image, then insertion by slot inside an image)
    int* beg = new int[n_images + 1]();
    for (int v = 0; v < n_views; v++) {
        const dafne_tta_view& t = views[v];
        if (!t.d_rows || !t.d_count || t.tile < 0 || t.tile >= n_images || t.slot < 0 || (t.flip_x != 0 && t.flip_x != 1) ||
            (t.flip_y != 0 && t.flip_y != 1)) {
            delete[] beg;
            return dafne::fail(DAFNE_E_INVALID, "tta_candidates: view %d: image %d slot %d flips %d/%d", v, t.tile, t.slot,
                               t.flip_x, t.flip_y);
        }
        beg[t.tile + 1]++;
    }
    int nv_max = 0;
    for (int i = 0; i < n_images; i++) {
        nv_max = beg[i + 1] > nv_max ? beg[i + 1] : nv_max;
        beg[i + 1] += beg[i];
    }
    if ((long long)nv_max * k_cap > m_cap) {
        delete[] beg;
        return dafne::fail(DAFNE_E_INVALID, "tta_candidates: %d views x k_cap %d exceed m_cap %d", nv_max, k_cap, m_cap);
    }
    const size_t vbytes = dafne::align_up(sizeof(dafne_tta_view) * (size_t)n_views, 256);
    uint8_t* blob = new uint8_t[need]();
    dafne_tta_view* td = reinterpret_cast<dafne_tta_view*>(blob);
    int* fill = new int[n_images]();
    int rc = DAFNE_OK;
    for (int v = 0; v < n_views && rc == DAFNE_OK; v++) {
        const dafne_tta_view& t = views[v];
        int p = beg[t.tile] + fill[t.tile]++;
        while (p > beg[t.tile] && td[p - 1].slot >= t.slot) {
            if (td[p - 1].slot == t.slot) rc = dafne::fail(DAFNE_E_INVALID, "tta_candidates: image %d has slot %d twice", t.tile, t.slot);
            td[p] = td[p - 1];
            p--;
        }
        td[p] = t;
    }
    delete[] fill;
    if (rc == DAFNE_OK) memcpy(blob + vbytes, beg, sizeof(int) * ((size_t)n_images + 1));
    delete[] beg;
    if (rc != DAFNE_OK) {
        delete[] blob;
        return rc;
    }
    hipStream_t st = (hipStream_t)stream;
    const hipError_t ce = hipMemcpyAsync(d_ws, blob, need, hipMemcpyHostToDevice, st);
    delete[] blob;
    if (ce != hipSuccess) return dafne::fail(DAFNE_E_HIP, "tta_candidates: hipMemcpyAsync: %s", hipGetErrorString(ce));
    hipLaunchKernelGGL(tta_candidates_kernel, dim3(n_images, nv_max > 0 ? nv_max : 1), dim3(256), 0, st, (const dafne_tta_view*)d_ws,
                       (const int*)((uint8_t*)d_ws + vbytes), k_cap, m_cap, d_corners, d_scores, d_ctr, d_classes, d_locs,
                       d_levels, d_hbox, d_counts, d_overflow);
    return dafne::check_launch("tta_candidates");
}

}  // extern "C"

// ------------------------------------------------ target assignment and loss values (dafne_assign_targets_hip, dafne_losses_hip)
#include "targets_kernels.h"

// ------------------------------------------------ scene labels -> tile ground truth (dafne_scene_split_labels_hip, dafne_scene_pack_tile_gt_hip)
#include "scene_labels_kernels.h"

// ------------------------------------------------ ground truth of training views (dafne_train_gt_hip)
#include "train_views_kernels.h"

// ------------------------------------------------ back through the finished regressions (dafne_head_uncook_backward_hip)
#include "pred_backward_kernels.h"

// ------------------------------------------------ SGD step that writes the packed weights in place (dafne_sgd_step_hip)
#include "solver_kernels.h"
