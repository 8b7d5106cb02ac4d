// aug_geom.h -- device code shared by the two training-augmentation sources (pcaug.hip: KITTI PointPillars, cpaug.hip: CenterPoint):
// the BEV rectangle, the collision predicate of box_collision_test (quirk (a) of include/minddet_hip_pcaug.h) and the sample of a row (the
// stable compaction of the rows is workgroup.h's).  Include it after
// `#pragma clang fp contract(off)`: every expression here is evaluated as written.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#pragma clang fp contract(off)

namespace md {

// corners of the (w, l) rectangle rotated by the angle whose cosine / sine are c / s, in the reference's order (box2d_to_corner_jit,
// box_np_ops.py:340-360: (-,-), (-,+), (+,+), (+,-) halves; row vector times [[c, -s], [s, c]]), about (0, 0)
__device__ __forceinline__ void rect_corners(double w, double l, double c, double s, double *x, double *y) {
    const double nx[4] = {-0.5, -0.5, 0.5, 0.5}, ny[4] = {-0.5, 0.5, 0.5, -0.5};
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const double px = nx[m] * w, py = ny[m] * l;
        x[m] = px * c + py * s;
        y[m] = -px * s + py * c;
    }
}

// _get_box_overlap_another (:769-785), clockwise: every corner of Q strictly on the inner side of every edge of P
__device__ __forceinline__ bool covers(const double *px, const double *py, const double *qx, const double *qy) {
    for (int m = 0; m < 4; ++m)
        for (int k = 0; k < 4; ++k) {
            const int k1 = (k + 1) & 3;
            const double vx = -(px[k] - px[k1]), vy = -(py[k] - py[k1]);
            double cross = vy * (px[k] - qx[m]);
            cross -= vx * (py[k] - qy[m]);
            if (cross >= 0) return false;
        }
    return true;
}

// box_collision_test (:708-746) for one pair, quirk (a) read as the text means it
__device__ __forceinline__ bool collide(const double *ax, const double *ay, const double *bx, const double *by) {
    const double aminx = fmin(fmin(ax[0], ax[1]), fmin(ax[2], ax[3])), amaxx = fmax(fmax(ax[0], ax[1]), fmax(ax[2], ax[3]));
    const double aminy = fmin(fmin(ay[0], ay[1]), fmin(ay[2], ay[3])), amaxy = fmax(fmax(ay[0], ay[1]), fmax(ay[2], ay[3]));
    const double bminx = fmin(fmin(bx[0], bx[1]), fmin(bx[2], bx[3])), bmaxx = fmax(fmax(bx[0], bx[1]), fmax(bx[2], bx[3]));
    const double bminy = fmin(fmin(by[0], by[1]), fmin(by[2], by[3])), bmaxy = fmax(fmax(by[0], by[1]), fmax(by[2], by[3]));
    const double iw = fmin(amaxx, bmaxx) - fmax(aminx, bminx), ih = fmin(amaxy, bmaxy) - fmax(aminy, bminy);
    if (!(ih > 0 && iw > 0)) return false;
    for (int k = 0; k < 4; ++k)          // _get_ret (:749-766)
        for (int m = 0; m < 4; ++m) {
            const double a0 = ax[k], a1 = ay[k], b0 = ax[(k + 1) & 3], b1 = ay[(k + 1) & 3];
            const double c0 = bx[m], c1 = by[m], d0 = bx[(m + 1) & 3], d1 = by[(m + 1) & 3];
            const bool acd = (d1 - a1) * (c0 - a0) > (c1 - a1) * (d0 - a0);
            const bool bcd = (d1 - b1) * (c0 - b0) > (c1 - b1) * (d0 - b0);
            if (acd != bcd) {
                const bool abc = (c1 - a1) * (b0 - a0) > (b1 - a1) * (c0 - a0);
                const bool abd = (d1 - a1) * (b0 - a0) > (b1 - a1) * (d0 - a0);
                if (abc != abd) return true;
            }
        }
    return covers(ax, ay, bx, by) || covers(bx, by, ax, ay);
}

// the sample of row i, or -1: a binary search of offsets[0 .. B] where it lies (at most 13 reads of a table every workgroup shares)
__device__ __forceinline__ int find_sample(const int *__restrict__ offsets, int B, int i) {
    int lo = 0, hi = B + 1;                 // first index whose offset is above i
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (offsets[mid] > i) hi = mid; else lo = mid + 1;
    }
    return (lo == 0 || lo == B + 1) ? -1 : lo - 1;
}

}  // namespace md
