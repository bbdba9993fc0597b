// Scene labels -> the ground truth of every tile of a split scene, for gfx950 (dafne_scene_split_labels_hip,
// dafne_scene_pack_tile_gt_hip): ImgSplit_multi_process.splitbase.savepatches (tools/prepare_dota, :147-207) for convex
// quadrilaterals, then the training filter of DOTA2COCO.py:49 and dafne/data/datasets/dota.py:226, :247-264.
//
//   split_kernel     one thread per (tile, object of the tile's scene) pair; pairs are tile-major, a tile's pairs in the
//                    scene's label-file order.  Everything in fp64, every operation singly and in this order (the unit is
//                    compiled with -ffp-contract=off; / and __dsqrt_rn are correctly rounded):
//                      1. the object's corners p0..p3 = trunc(label value)            (parse_dota_poly2's int())
//                      2. cr_i = (p(i+1).x - p_i.x) (p(i+2).y - p(i+1).y) - (p(i+1).y - p_i.y) (p(i+2).x - p(i+1).x), i = 0..3;
//                         a positive and a negative one: NONCONVEX (shapely raises on such a ring; the one deviation)
//                      3. shoelace(q) = sum_i (x_i y_(i+1) - x_(i+1) y_i) added in index order from 0.0;
//                         area = |shoelace(p)| * 0.5; not > 0: NONE
//                      4. all corners in [left, right] x [up, down]: INSIDE, row = int(p - origin), difficult unchanged
//                      5. Sutherland-Hodgman against x >= left, x <= right, y >= up, y <= down in that order; per edge,
//                         for i = 0..n-1 with c = q_i, p = q_(i-1) (cyclic): c inside: [cut(p, c) if p outside], c;
//                         else [cut(p, c) if p inside].  cut on x = v: t = (v - p.x) / (c.x - p.x), (v, p.y + t (c.y - p.y));
//                         on y = v: t = (v - p.y) / (c.y - p.y), (p.x + t (c.x - p.x), v).  Then consecutive equal vertices
//                         are merged (also last = first).  Fewer than 3 left: NONE.
//                         half = (|shoelace(q)| * 0.5) / area; not > 0: NONE
//                      6. shoelace(q) < 0: q = q0, q(n-1), .., q1                       (orient(sign=1) keeps the start vertex)
//                         n < 4: DROP_LT4; n > 5: DROP_GT5
//                      7. n == 5 (CUT5): d_i = sqrt(dx dx + dy dy) of q_i - q_((i+1) % 5); the first minimal edge `pos` is
//                         replaced by ((a.x + b.x) / 2, (a.y + b.y) / 2) in GetPoly4FromPoly5's emission order
//                      8. over the cyclic shifts k = 0..3: e = (q_((i+k) % 4) - p_i)^2 per coordinate,
//                         dist = ((e0 + e1) + (e2 + e3)) + ((e4 + e5) + (e6 + e7)) (numpy's sum of eight); first minimum
//                      9. row = int(q - origin)   10. row <= 1 -> 1, >= patch -> patch   11. difficult = half > thresh ? own : 2
//                    kept (the training filter, on the integer row): difficult != 2, |shoelace| * 0.5 > min_area,
//                    max(bbox w, bbox h) >= min_side, no two corners with |dx| + |dy| < 1e-2.
//   count_kernel     one wavefront per tile: outcome counts, written rows, kept rows (lane sums, xor-shuffle reduction)
//   scan_kernel      one wavefront: exclusive scans of the two per-tile counts (shuffle scan, 64 tiles a step, running
//                    carry) -> offsets [T + 1]; the outcome totals
//   write_kernel     one wavefront per tile: a row's position = its tile's offset + rows before it in the tile (ballot +
//                    popcount).  Ordered, no atomics: equal bits from run to run.
//
// This text is compiled as part of decode.hip (its last #include), like targets_kernels.h: one matrix-free translation unit
// with -ffp-contract=off -fno-slp-vectorize under the static packed-fp32 rule (tests/test_packed_fp32.py).
#pragma once
#include "common.h"
#include "sort_quad.h"

namespace {
namespace scene_labels {

constexpr int kRec = 12;         // outcome, 8 tile coordinates, difficult, kept, 0
constexpr int kCounts = 9;       // 7 outcomes, written rows, kept rows
constexpr int kMaxV = 8;         // a quadrilateral cut by four half-planes has at most 8 vertices
enum { NONE = 0, INSIDE = 1, CUT4 = 2, CUT5 = 3, DROP_LT4 = 4, DROP_GT5 = 5, NONCONVEX = 6 };

struct SplitArgs {
    const int32_t* tiles;        // [T, 5] scene, left, up, right, down
    const int32_t* pair_off;     // [T + 1]
    const int32_t* obj_off;      // [S + 1]
    const double* boxes;         // [G, 8]
    const int32_t* difficult;    // [G]
    int32_t* rec;                // [P, 12]
    int n_tiles, n_objects, n_pairs, patch;
    double thresh, min_area, min_side;
};

__device__ inline double shoelace(const double* x, const double* y, int n) {
    double s = 0.0;
    for (int i = 0; i < n; i++) {
        const int j = i + 1 == n ? 0 : i + 1;
        s = s + (x[i] * y[j] - x[j] * y[i]);
    }
    return s;
}

__device__ inline bool inside_edge(int edge, double x, double y, double v) {
    return edge == 0 ? x >= v : edge == 1 ? x <= v : edge == 2 ? y >= v : y <= v;
}

// one Sutherland-Hodgman pass; returns the new vertex count (never above kMaxV: vertices past it are not stored)
__device__ inline int clip_edge(const double* ix, const double* iy, int n, int edge, double v, double* ox, double* oy) {
    int m = 0;
    for (int i = 0; i < n; i++) {
        const int h = i == 0 ? n - 1 : i - 1;
        const double cx = ix[i], cy = iy[i], px = ix[h], py = iy[h];
        const bool cin = inside_edge(edge, cx, cy, v), pin = inside_edge(edge, px, py, v);
        if (cin != pin) {
            double qx, qy;
            if (edge < 2) {
                const double t = (v - px) / (cx - px);
                qx = v;
                qy = py + t * (cy - py);
            } else {
                const double t = (v - py) / (cy - py);
                qx = px + t * (cx - px);
                qy = v;
            }
            if (m < kMaxV) { ox[m] = qx; oy[m] = qy; m++; }
        }
        if (cin && m < kMaxV) { ox[m] = cx; oy[m] = cy; m++; }
    }
    return m;
}

__device__ inline int trunc_to_int(double v) { return (int)v; }   // C conversion truncates toward zero, like int()

__device__ inline bool keep_row(const int* r, int difficult, double min_area, double min_side) {
    if (difficult == 2) return false;
    double x[4], y[4];
    for (int i = 0; i < 4; i++) { x[i] = (double)r[2 * i]; y[i] = (double)r[2 * i + 1]; }
    if (!(fabs(shoelace(x, y, 4)) * 0.5 > min_area)) return false;
    const double w = fmax(fmax(x[0], x[1]), fmax(x[2], x[3])) - fmin(fmin(x[0], x[1]), fmin(x[2], x[3]));
    const double h = fmax(fmax(y[0], y[1]), fmax(y[2], y[3])) - fmin(fmin(y[0], y[1]), fmin(y[2], y[3]));
    if (!(fmax(w, h) >= min_side)) return false;
    for (int i = 0; i < 4; i++)
        for (int j = i + 1; j < 4; j++)
            if (fabs(x[i] - x[j]) + fabs(y[i] - y[j]) < 1e-2) return false;
    return true;
}

__global__ void __launch_bounds__(256) split_kernel(SplitArgs a) {
    const long long gp = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gp >= a.n_pairs) return;
    const int p = (int)gp;
    // the tile of pair p: the last t with pair_off[t] <= p (tiles of a scene without objects have no pairs)
    int lo = 0, hi = a.n_tiles;
    while (hi - lo > 1) {
        const int mid = lo + (hi - lo) / 2;
        if (a.pair_off[mid] <= p) lo = mid; else hi = mid;
    }
    const int t = lo;
    const int32_t* td = a.tiles + (size_t)t * 5;
    const int g = a.obj_off[td[0]] + (p - a.pair_off[t]);
    int32_t* rec = a.rec + (size_t)p * kRec;
    int code = NONE, diff = 0, kept = 0;
    int row[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (g >= 0 && g < a.n_objects) {
        const double left = (double)td[1], up = (double)td[2], right = (double)td[3], down = (double)td[4];
        double ox[4], oy[4];
        for (int i = 0; i < 4; i++) {
            ox[i] = trunc(a.boxes[(size_t)g * 8 + 2 * i]);
            oy[i] = trunc(a.boxes[(size_t)g * 8 + 2 * i + 1]);
        }
        const int own = a.difficult[g];
        bool pos = false, neg = false, all_in = true;
        for (int i = 0; i < 4; i++) {
            const int j = (i + 1) & 3, k = (i + 2) & 3;
            const double cr = (ox[j] - ox[i]) * (oy[k] - oy[j]) - (oy[j] - oy[i]) * (ox[k] - ox[j]);
            pos = pos || cr > 0.0;
            neg = neg || cr < 0.0;
            all_in = all_in && ox[i] >= left && ox[i] <= right && oy[i] >= up && oy[i] <= down;
        }
        const double area = fabs(shoelace(ox, oy, 4)) * 0.5;
        if (pos && neg) {
            code = NONCONVEX;
        } else if (!(area > 0.0)) {
            code = NONE;
        } else if (all_in) {
            code = INSIDE;
            diff = own;
            for (int i = 0; i < 4; i++) {
                row[2 * i] = trunc_to_int(ox[i] - left);
                row[2 * i + 1] = trunc_to_int(oy[i] - up);
            }
        } else {
            double ax[kMaxV], ay[kMaxV], bx[kMaxV], by[kMaxV];
            int n = clip_edge(ox, oy, 4, 0, left, ax, ay);
            n = clip_edge(ax, ay, n, 1, right, bx, by);
            n = clip_edge(bx, by, n, 2, up, ax, ay);
            n = clip_edge(ax, ay, n, 3, down, bx, by);
            int m = 0;      // merge consecutive equal vertices into a*
            for (int i = 0; i < n; i++)
                if (m == 0 || !(bx[i] == ax[m - 1] && by[i] == ay[m - 1])) { ax[m] = bx[i]; ay[m] = by[i]; m++; }
            if (m > 1 && ax[0] == ax[m - 1] && ay[0] == ay[m - 1]) m--;
            n = m;
            double half = 0.0, s = 0.0;
            if (n >= 3) {
                s = shoelace(ax, ay, n);
                half = (fabs(s) * 0.5) / area;
            }
            if (!(half > 0.0)) {
                code = NONE;
            } else if (n < 4) {
                code = DROP_LT4;
            } else if (n > 5) {
                code = DROP_GT5;
            } else {
                double qx[5], qy[5];
                for (int i = 0; i < n; i++) {      // orientation: a negative ring is walked backwards from its start vertex
                    const int src = (s < 0.0 && i > 0) ? n - i : i;
                    qx[i] = ax[src]; qy[i] = ay[src];
                }
                code = CUT4;
                if (n == 5) {
                    code = CUT5;
                    int pos5 = 0;
                    double dmin = 0.0;
                    for (int i = 0; i < 5; i++) {
                        const int j = i == 4 ? 0 : i + 1;
                        const double dx = qx[i] - qx[j], dy = qy[i] - qy[j];
                        const double d = __dsqrt_rn(dx * dx + dy * dy);
                        if (i == 0 || d < dmin) { dmin = d; pos5 = i; }
                    }
                    double rx4[4], ry4[4];
                    int m4 = 0;
                    const int skip = pos5 == 4 ? 0 : pos5 + 1;
                    for (int c = 0; c < 5; c++) {
                        if (c == pos5) {
                            const int j = c == 4 ? 0 : c + 1;
                            rx4[m4] = (qx[c] + qx[j]) / 2.0;
                            ry4[m4] = (qy[c] + qy[j]) / 2.0;
                            m4++;
                        } else if (c != skip) {
                            rx4[m4] = qx[c]; ry4[m4] = qy[c];
                            m4++;
                        }
                    }
                    for (int i = 0; i < 4; i++) { qx[i] = rx4[i]; qy[i] = ry4[i]; }
                }
                int best = 0;
                double bd = 0.0;
                for (int k = 0; k < 4; k++) {
                    double e[8];
                    for (int i = 0; i < 4; i++) {
                        const int src = (i + k) & 3;
                        const double ex = qx[src] - ox[i], ey = qy[src] - oy[i];
                        e[2 * i] = ex * ex;
                        e[2 * i + 1] = ey * ey;
                    }
                    const double dist = ((e[0] + e[1]) + (e[2] + e[3])) + ((e[4] + e[5]) + (e[6] + e[7]));
                    if (k == 0 || dist < bd) { bd = dist; best = k; }
                }
                for (int i = 0; i < 4; i++) {
                    const int src = (i + best) & 3;
                    int vx = trunc_to_int(qx[src] - left), vy = trunc_to_int(qy[src] - up);
                    vx = vx <= 1 ? 1 : (vx >= a.patch ? a.patch : vx);
                    vy = vy <= 1 ? 1 : (vy >= a.patch ? a.patch : vy);
                    row[2 * i] = vx;
                    row[2 * i + 1] = vy;
                }
                diff = half > a.thresh ? own : 2;
            }
        }
        if (code == INSIDE || code == CUT4 || code == CUT5) kept = keep_row(row, diff, a.min_area, a.min_side) ? 1 : 0;
    }
    rec[0] = code;
    for (int i = 0; i < 8; i++) rec[1 + i] = row[i];
    rec[9] = diff;
    rec[10] = kept;
    rec[11] = 0;
}

__device__ inline int wave_sum(int v) {
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// grid = T blocks of 64 threads (one wavefront)
__global__ void __launch_bounds__(64) count_kernel(const int32_t* rec, const int32_t* pair_off, int32_t* counts) {
    const int t = blockIdx.x, lane = threadIdx.x;
    const int p0 = pair_off[t], n = pair_off[t + 1] - p0;
    int c[kCounts];
    for (int i = 0; i < kCounts; i++) c[i] = 0;
    for (int j0 = 0; j0 < n; j0 += 64) {
        const int j = j0 + lane;
        if (j < n) {
            const int32_t* r = rec + (size_t)(p0 + j) * kRec;
            const int code = r[0];
            for (int i = 0; i < 7; i++) c[i] += code == i ? 1 : 0;
            const bool written = code == INSIDE || code == CUT4 || code == CUT5;
            c[7] += written ? 1 : 0;
            c[8] += (written && r[10] != 0) ? 1 : 0;
        }
    }
    for (int i = 0; i < kCounts; i++) {
        const int s = wave_sum(c[i]);
        if (lane == 0) counts[(size_t)t * kCounts + i] = s;
    }
}

// one block of 64 threads
__global__ void __launch_bounds__(64) scan_kernel(const int32_t* counts, int n_tiles, int32_t* all_off, int32_t* kept_off,
                                                  int32_t* stats) {
    const int lane = threadIdx.x;
    int carry_a = 0, carry_k = 0;
    int st[7] = {0, 0, 0, 0, 0, 0, 0};
    for (int base = 0; base < n_tiles; base += 64) {
        const int t = base + lane;
        const bool ok = t < n_tiles;
        const int ca = ok ? counts[(size_t)t * kCounts + 7] : 0, ck = ok ? counts[(size_t)t * kCounts + 8] : 0;
        for (int i = 0; i < 7; i++) st[i] += ok ? counts[(size_t)t * kCounts + i] : 0;
        int sa = ca, sk = ck;
        for (int d = 1; d < 64; d <<= 1) {
            const int ua = __shfl_up(sa, d, 64), uk = __shfl_up(sk, d, 64);
            if (lane >= d) { sa += ua; sk += uk; }
        }
        if (ok) {
            all_off[t] = carry_a + sa - ca;
            kept_off[t] = carry_k + sk - ck;
        }
        carry_a += __shfl(sa, 63, 64);
        carry_k += __shfl(sk, 63, 64);
    }
    for (int i = 0; i < 7; i++) {
        const int s = wave_sum(st[i]);
        if (lane == 0) stats[i] = s;
    }
    if (lane == 0) {
        all_off[n_tiles] = carry_a;
        kept_off[n_tiles] = carry_k;
        stats[7] = carry_a;
        stats[8] = carry_k;
    }
}

struct WriteArgs {
    const int32_t* rec;
    const int32_t* pair_off;
    const int32_t* tiles;
    const int32_t* obj_off;
    const int32_t* cls;
    const int32_t* all_off;
    const int32_t* kept_off;
    int32_t *all_corners, *all_class, *all_diff, *all_src;
    float *kept_corners, *kept_hbox, *kept_area;
    int32_t *kept_class, *kept_src;
    double rx, ry;
    int sort;
};

// grid = T blocks of 64 threads (one wavefront)
__global__ void __launch_bounds__(64) write_kernel(WriteArgs a) {
    const int t = blockIdx.x, lane = threadIdx.x;
    const int p0 = a.pair_off[t], n = a.pair_off[t + 1] - p0;
    const int g0 = a.obj_off[a.tiles[(size_t)t * 5]];
    int base_a = a.all_off[t], base_k = a.kept_off[t];
    const unsigned long long below = lane == 0 ? 0ull : (~0ull >> (64 - lane));
    for (int j0 = 0; j0 < n; j0 += 64) {      // n is the same in every lane: all of them reach the ballots
        const int j = j0 + lane;
        const int32_t* r = a.rec + (size_t)(p0 + (j < n ? j : 0)) * kRec;
        const int code = j < n ? r[0] : NONE;
        const bool written = code == INSIDE || code == CUT4 || code == CUT5;
        const bool kept = written && r[10] != 0;
        const unsigned long long ma = __ballot(written), mk = __ballot(kept);
        const int g = g0 + j;
        if (written) {
            const size_t o = (size_t)base_a + __popcll(ma & below);
            for (int i = 0; i < 8; i++) a.all_corners[o * 8 + i] = r[1 + i];
            a.all_class[o] = a.cls[g];
            a.all_diff[o] = r[9];
            a.all_src[o] = g;
        }
        if (kept) {
            const size_t o = (size_t)base_k + __popcll(mk & below);
            float q[8];
            for (int i = 0; i < 4; i++) {      // gt_instances_from_objects: fp64 product, one rounding to fp32
                q[2 * i] = (float)((double)r[1 + 2 * i] * a.rx);
                q[2 * i + 1] = (float)((double)r[2 + 2 * i] * a.ry);
            }
            if (a.sort) dafne::sort_quad(q);
            for (int i = 0; i < 8; i++) a.kept_corners[o * 8 + i] = q[i];
            a.kept_hbox[o * 4 + 0] = fminf(fminf(q[0], q[2]), fminf(q[4], q[6]));
            a.kept_hbox[o * 4 + 1] = fminf(fminf(q[1], q[3]), fminf(q[5], q[7]));
            a.kept_hbox[o * 4 + 2] = fmaxf(fmaxf(q[0], q[2]), fmaxf(q[4], q[6]));
            a.kept_hbox[o * 4 + 3] = fmaxf(fmaxf(q[1], q[3]), fmaxf(q[5], q[7]));
            // data.targets.polygon_area: two sums of four fp64 products in index order, 0.5 |difference|, one rounding
            double s1 = 0.0, s2 = 0.0;
            for (int i = 0; i < 4; i++) {
                const int k = (i + 1) & 3;
                s1 = s1 + (double)q[2 * i] * (double)q[2 * k + 1];
                s2 = s2 + (double)q[2 * i + 1] * (double)q[2 * k];
            }
            a.kept_area[o] = (float)(0.5 * fabs(s1 - s2));
            a.kept_class[o] = a.cls[g];
            a.kept_src[o] = g;
        }
        base_a += __popcll(ma);
        base_k += __popcll(mk);
    }
}

}  // namespace scene_labels
}  // namespace

extern "C" {

int dafne_scene_split_labels_hip(const int32_t* d_tiles5, const int32_t* d_pair_off, int n_tiles, const int32_t* d_obj_off,
                                 int n_scenes, const double* d_boxes, const int32_t* d_difficult, int n_objects, int patch,
                                 double thresh, double min_area, double min_side, int32_t* d_records, int64_t n_pairs,
                                 void* stream) {
    using namespace scene_labels;
    if (n_tiles < 0 || n_scenes < 0 || n_objects < 0 || n_pairs < 0 || patch < 1)
        return dafne::fail(DAFNE_E_INVALID, "scene_split_labels: negative size or patch < 1");
    if (n_pairs > 2147483647LL)
        return dafne::fail(DAFNE_E_INVALID, "scene_split_labels: %lld (tile, object) pairs overflow the int32 pair index",
                           (long long)n_pairs);
    if (n_pairs == 0) return DAFNE_OK;
    if (!d_tiles5 || !d_pair_off || !d_obj_off || !d_boxes || !d_difficult || !d_records || n_tiles == 0 || n_objects == 0)
        return dafne::fail(DAFNE_E_INVALID, "scene_split_labels: null pointer or pairs without tiles / objects");
    SplitArgs a;
    a.tiles = d_tiles5; a.pair_off = d_pair_off; a.obj_off = d_obj_off; a.boxes = d_boxes; a.difficult = d_difficult;
    a.rec = d_records; a.n_tiles = n_tiles; a.n_objects = n_objects; a.n_pairs = (int)n_pairs; a.patch = patch;
    a.thresh = thresh; a.min_area = min_area; a.min_side = min_side;
    const unsigned blocks = (unsigned)((n_pairs + 255) / 256);
    hipLaunchKernelGGL(split_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, a);
    return dafne::check_launch("scene_labels::split_kernel");
}

size_t dafne_scene_pack_tile_gt_workspace_bytes(int n_tiles) {
    return n_tiles <= 0 ? 256 : dafne::align_up((size_t)n_tiles * scene_labels::kCounts * sizeof(int32_t), 256);
}

int dafne_scene_pack_tile_gt_hip(const int32_t* d_records, const int32_t* d_pair_off, const int32_t* d_tiles5, int n_tiles,
                                 const int32_t* d_obj_off, const int32_t* d_class, double ratio_x, double ratio_y, int sort,
                                 int32_t* d_all_offsets, int32_t* d_all_corners, int32_t* d_all_class, int32_t* d_all_difficult,
                                 int32_t* d_all_src, int32_t* d_kept_offsets, float* d_kept_corners, float* d_kept_hbox,
                                 float* d_kept_area, int32_t* d_kept_class, int32_t* d_kept_src, int32_t* d_stats9, void* d_ws,
                                 size_t ws_bytes, void* stream) {
    using namespace scene_labels;
    if (n_tiles < 1) return dafne::fail(DAFNE_E_INVALID, "scene_pack_tile_gt: no tiles");
    if (!d_records || !d_pair_off || !d_tiles5 || !d_obj_off || !d_class || !d_all_offsets || !d_all_corners || !d_all_class ||
        !d_all_difficult || !d_all_src || !d_kept_offsets || !d_kept_corners || !d_kept_hbox || !d_kept_area || !d_kept_class ||
        !d_kept_src || !d_stats9 || !d_ws)
        return dafne::fail(DAFNE_E_INVALID, "scene_pack_tile_gt: null pointer");
    if (ws_bytes < dafne_scene_pack_tile_gt_workspace_bytes(n_tiles))
        return dafne::fail(DAFNE_E_WORKSPACE, "scene_pack_tile_gt: workspace of %zu bytes, %zu needed", ws_bytes,
                           dafne_scene_pack_tile_gt_workspace_bytes(n_tiles));
    hipStream_t st = (hipStream_t)stream;
    int32_t* counts = static_cast<int32_t*>(d_ws);
    hipLaunchKernelGGL(count_kernel, dim3(n_tiles), dim3(64), 0, st, d_records, d_pair_off, counts);
    if (int rc = dafne::check_launch("scene_labels::count_kernel")) return rc;
    hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(64), 0, st, counts, n_tiles, d_all_offsets, d_kept_offsets, d_stats9);
    if (int rc = dafne::check_launch("scene_labels::scan_kernel")) return rc;
    WriteArgs a;
    a.rec = d_records; a.pair_off = d_pair_off; a.tiles = d_tiles5; a.obj_off = d_obj_off; a.cls = d_class;
    a.all_off = d_all_offsets; a.kept_off = d_kept_offsets;
    a.all_corners = d_all_corners; a.all_class = d_all_class; a.all_diff = d_all_difficult; a.all_src = d_all_src;
    a.kept_corners = d_kept_corners; a.kept_hbox = d_kept_hbox; a.kept_area = d_kept_area; a.kept_class = d_kept_class;
    a.kept_src = d_kept_src; a.rx = ratio_x; a.ry = ratio_y; a.sort = sort;
    hipLaunchKernelGGL(write_kernel, dim3(n_tiles), dim3(64), 0, st, a);
    return dafne::check_launch("scene_labels::write_kernel");
}

}  // extern "C"
