// sort_quadrilateral (dafne/utils/sort_corners.py:26-92) as a device function, shared by decode.hip (decoded boxes) and
// targets_kernels.h (predicted corners of positive locations).  fp32 in the reference's operation order: include it only from
// units compiled with -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>

namespace dafne {

__device__ __forceinline__ float pick4(float a, float b, float c, float d, int i) {
    float r = a;
    if (i == 1) r = b;
    if (i == 2) r = c;
    if (i == 3) r = d;
    return r;
}

__device__ __forceinline__ float cross2(float ax, float ay, float bx, float by) {
    return ax * by - ay * bx;   // sort_corners.py:5-7 (two products, one subtraction)
}

// sort_corners.py:26-92, one box per call; q = x0,y0,..,x3,y3 in place.
__device__ inline void sort_quad(float* q) {
    const float x0 = q[0], y0 = q[1], x1 = q[2], y1 = q[3], x2 = q[4], y2 = q[5], x3 = q[6], y3 = q[7];
    int k1 = 0;   // first vertex of minimal x (:46)
    float mx = x0;
    if (x1 < mx) { mx = x1; k1 = 1; }
    if (x2 < mx) { mx = x2; k1 = 2; }
    if (x3 < mx) { mx = x3; k1 = 3; }
    const float p1x = pick4(x0, x1, x2, x3, k1), p1y = pick4(y0, y1, y2, y3, k1);
    float rx[3], ry[3];
#pragma unroll
    for (int j = 0; j < 3; j++) {
        int src = j < k1 ? j : j + 1;
        rx[j] = pick4(x0, x1, x2, x3, src);
        ry[j] = pick4(y0, y1, y2, y3, src);
    }
    float p3x = 0.f, p3y = 0.f, ax = 0.f, ay = 0.f, bx = 0.f, by = 0.f;
    bool done = false;
#pragma unroll
    for (int i = 0; i < 3; i++) {   // :57-73
        const int i2 = i == 0 ? 1 : 0, i3 = i == 2 ? 1 : 2;
        const float dx = rx[i] - p1x, dy = ry[i] - p1y;
        const float l = cross2(dx, dy, rx[i2] - p1x, ry[i2] - p1y);
        const float r = cross2(dx, dy, rx[i3] - p1x, ry[i3] - p1y);
        const bool cond = (l * r < 0.0f) && !done;
        if (cond) {
            p3x = rx[i]; p3y = ry[i];
            ax = rx[i2]; ay = ry[i2];
            bx = rx[i3]; by = ry[i3];
        }
        done = done || cond;
    }
    // :77-90: iteration 0 tests A, iteration 1 tests B unless A already matched
    const float ex = p3x - p1x, ey = p3y - p1y;
    const bool c0 = cross2(ex, ey, ax - p1x, ay - p1y) > 0.0f;
    const bool c1 = cross2(ex, ey, bx - p1x, by - p1y) > 0.0f;
    const bool swap = !c0 && c1;
    q[0] = p1x; q[1] = p1y;
    q[2] = swap ? bx : ax; q[3] = swap ? by : ay;
    q[4] = p3x; q[5] = p3y;
    q[6] = swap ? ax : bx; q[7] = swap ? ay : by;
}

// sort_quad with the selection made visible: src[j] = the input corner that output corner j was copied from, or -1 where the
// reference leaves its new_zeros (no l * r < 0 among the three candidates: collinear or coinciding points), which is where the
// reference's autograd sends no gradient.  Same comparisons in the same order as sort_quad; q gets the same values.
__device__ inline void sort_quad_src(float* q, int* src) {
    const float x0 = q[0], y0 = q[1], x1 = q[2], y1 = q[3], x2 = q[4], y2 = q[5], x3 = q[6], y3 = q[7];
    int k1 = 0;
    float mx = x0;
    if (x1 < mx) { mx = x1; k1 = 1; }
    if (x2 < mx) { mx = x2; k1 = 2; }
    if (x3 < mx) { mx = x3; k1 = 3; }
    const float p1x = pick4(x0, x1, x2, x3, k1), p1y = pick4(y0, y1, y2, y3, k1);
    float rx[3], ry[3];
    int rs[3];
#pragma unroll
    for (int j = 0; j < 3; j++) {
        rs[j] = j < k1 ? j : j + 1;
        rx[j] = pick4(x0, x1, x2, x3, rs[j]);
        ry[j] = pick4(y0, y1, y2, y3, rs[j]);
    }
    float p3x = 0.f, p3y = 0.f, ax = 0.f, ay = 0.f, bx = 0.f, by = 0.f;
    int s3 = -1, sa = -1, sb = -1;
    bool done = false;
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const int i2 = i == 0 ? 1 : 0, i3 = i == 2 ? 1 : 2;
        const float dx = rx[i] - p1x, dy = ry[i] - p1y;
        const float l = cross2(dx, dy, rx[i2] - p1x, ry[i2] - p1y);
        const float r = cross2(dx, dy, rx[i3] - p1x, ry[i3] - p1y);
        const bool cond = (l * r < 0.0f) && !done;
        if (cond) {
            p3x = rx[i]; p3y = ry[i]; s3 = rs[i];
            ax = rx[i2]; ay = ry[i2]; sa = rs[i2];
            bx = rx[i3]; by = ry[i3]; sb = rs[i3];
        }
        done = done || cond;
    }
    const float ex = p3x - p1x, ey = p3y - p1y;
    const bool c0 = cross2(ex, ey, ax - p1x, ay - p1y) > 0.0f;
    const bool c1 = cross2(ex, ey, bx - p1x, by - p1y) > 0.0f;
    const bool swap = !c0 && c1;
    q[0] = p1x; q[1] = p1y;
    q[2] = swap ? bx : ax; q[3] = swap ? by : ay;
    q[4] = p3x; q[5] = p3y;
    q[6] = swap ? ax : bx; q[7] = swap ? ay : by;
    src[0] = k1;
    src[1] = swap ? sb : sa;
    src[2] = s3;
    src[3] = swap ? sa : sb;
}

}  // namespace dafne
