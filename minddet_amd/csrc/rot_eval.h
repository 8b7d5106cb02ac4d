// rot_eval.h -- the per-pair arithmetic of rotate_iou_kernel_eval (pointpillars/eval_gpu/rotate_iou.py:167-302), stated once: the
// numba.cuda rotated IoU with the point-in-quadrilateral + segment-intersection + pseudo-angle insertion sort formulation and the
// `criterion` switch.  md_rotate_iou_eval (nms.hip) and md_kitti_eval_overlaps (kittieval.hip) both call rie_pair, so the two give the
// same bits for the same pair.  Device code only.  fp32 without contraction: every function body says so itself, whatever the including
// file's setting is.  Polygon scratch is the caller's LDS: 3 * 24 floats per lane, slot-major with a stride of RIE_LANES floats.
#pragma once
#include <hip/hip_runtime.h>

namespace md {

constexpr int RIE_LANES = 256;                 // lanes of the calling workgroup = the stride between a lane's polygon slots
constexpr int RIE_PTS = 24;                    // polygon slots per lane
constexpr int RIE_LDS_FLOATS = 3 * RIE_PTS * RIE_LANES;
// The one departure from the reference.  When two edges are collinear (equal yaw, one shared edge line) its four strict orientation tests
// are decided by rounding, and where they say "crossing" the point is a quotient of two rounding residues: a vertex anywhere in the plane,
// an intersection of 672 m2 for two cars, an IoU of -34 (tests/rot_eval_contract.py has the figures).  A crossing lies on both segments,
// so a point is kept only if it is within tol = 2^-16 x the largest coordinate of the four end points of the extent of both segments and of
// both edge lines (NaN and infinity fail).  A point dropped wrongly would have to be that far off; one kept wrongly adds at most
// tol x edge length / 2 to the area, 2.6e-3 m2 for a car at 80 m.  Every non-coincident pair of the contract's generators keeps the bits
// it had without the test; among 112 522 further overlapping jittered pairs 5 changed, each a crossing of edges within 1.4e-3 rad of
// parallel that had left its segments, and each result moved towards the float64 geometric value (worst error 3.9e-3 -> 1.6e-4).
constexpr float RIE_CROSS_TOL = 1.52587890625e-05f;   // 2^-16

__device__ __forceinline__ void rie_corners(const float *rb, float *c) {
#pragma clang fp contract(off)
    const float a_cos = cosf(rb[4]), a_sin = sinf(rb[4]);
    const float cx[4] = {-rb[2] / 2, -rb[2] / 2, rb[2] / 2, rb[2] / 2};
    const float cy[4] = {-rb[3] / 2, rb[3] / 2, rb[3] / 2, -rb[3] / 2};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        c[2 * i] = a_cos * cx[i] + a_sin * cy[i] + rb[0];
        c[2 * i + 1] = -a_sin * cx[i] + a_cos * cy[i] + rb[1];
    }
}
__device__ __forceinline__ bool rie_in_quad(float px, float py, const float *c) {
#pragma clang fp contract(off)
    const float ab0 = c[2] - c[0], ab1 = c[3] - c[1], ad0 = c[6] - c[0], ad1 = c[7] - c[1];
    const float ap0 = px - c[0], ap1 = py - c[1];
    const float abab = ab0 * ab0 + ab1 * ab1, abap = ab0 * ap0 + ab1 * ap1;
    const float adad = ad0 * ad0 + ad1 * ad1, adap = ad0 * ap0 + ad1 * ap1;
    return abab >= abap && abap >= 0 && adad >= adap && adap >= 0;
}
// r1, r2: (x, y, w, h, angle) of the box and of the query box; scratch: the workgroup's RIE_LDS_FLOATS floats of LDS.
// criterion -1: IoU, 0: intersection / area of r1, 1: / area of r2, else the intersection area
__device__ __forceinline__ float rie_pair(const float *r1, const float *r2, int criterion, float *scratch) {
#pragma clang fp contract(off)
    float c1[8], c2[8];
    rie_corners(r1, c1);
    rie_corners(r2, c2);
    float *px = scratch + threadIdx.x, *py = px + RIE_PTS * RIE_LANES, *vs = py + RIE_PTS * RIE_LANES;
    int m = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (rie_in_quad(c1[2 * i], c1[2 * i + 1], c2)) { px[m * RIE_LANES] = c1[2 * i]; py[m * RIE_LANES] = c1[2 * i + 1]; ++m; }
        if (rie_in_quad(c2[2 * i], c2[2 * i + 1], c1)) { px[m * RIE_LANES] = c2[2 * i]; py[m * RIE_LANES] = c2[2 * i + 1]; ++m; }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float A0 = c1[2 * i], A1 = c1[2 * i + 1], B0 = c1[2 * ((i + 1) & 3)], B1 = c1[2 * ((i + 1) & 3) + 1];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float C0 = c2[2 * j], C1 = c2[2 * j + 1], D0 = c2[2 * ((j + 1) & 3)], D1 = c2[2 * ((j + 1) & 3) + 1];
            const float BA0 = B0 - A0, BA1 = B1 - A1, DA0 = D0 - A0, CA0 = C0 - A0, DA1 = D1 - A1, CA1 = C1 - A1;
            const bool acd = DA1 * CA0 > CA1 * DA0;
            const bool bcd = (D1 - B1) * (C0 - B0) > (C1 - B1) * (D0 - B0);
            if (acd != bcd) {
                const bool abc = CA1 * BA0 > BA1 * CA0, abd = DA1 * BA0 > BA1 * DA0;
                if (abc != abd && m < 24) {
                    const float DC0 = D0 - C0, DC1 = D1 - C1;
                    const float ABBA = A0 * B1 - B0 * A1, CDDC = C0 * D1 - D0 * C1;
                    const float DH = BA1 * DC0 - BA0 * DC1;
                    const float X = (ABBA * DC0 - BA0 * CDDC) / DH, Y = (ABBA * DC1 - BA1 * CDDC) / DH;
                    // the one departure from the reference: the crossing has to lie on both segments (RIE_CROSS_TOL)
                    const float mag = fmaxf(fmaxf(fmaxf(fabsf(A0), fabsf(A1)), fmaxf(fabsf(B0), fabsf(B1))),
                                            fmaxf(fmaxf(fabsf(C0), fabsf(C1)), fmaxf(fabsf(D0), fabsf(D1))));
                    const float tol = RIE_CROSS_TOL * mag;
                    if (X >= fmaxf(fminf(A0, B0), fminf(C0, D0)) - tol && X <= fminf(fmaxf(A0, B0), fmaxf(C0, D0)) + tol &&
                        Y >= fmaxf(fminf(A1, B1), fminf(C1, D1)) - tol && Y <= fminf(fmaxf(A1, B1), fmaxf(C1, D1)) + tol &&
                        fabsf(BA0 * (Y - A1) - BA1 * (X - A0)) <= tol * (fabsf(BA0) + fabsf(BA1)) &&
                        fabsf(DC0 * (Y - C1) - DC1 * (X - C0)) <= tol * (fabsf(DC0) + fabsf(DC1))) {
                        px[m * RIE_LANES] = X;
                        py[m * RIE_LANES] = Y;
                        ++m;
                    }
                }
            }
        }
    }
    float ai = 0.f;
    if (m > 0) {
        float cx = 0.f, cy = 0.f;
        for (int i = 0; i < m; ++i) { cx += px[i * RIE_LANES]; cy += py[i * RIE_LANES]; }
        cx /= (float)m;
        cy /= (float)m;
        for (int i = 0; i < m; ++i) {
            float v0 = px[i * RIE_LANES] - cx, v1 = py[i * RIE_LANES] - cy;
            const float d = sqrtf(v0 * v0 + v1 * v1);
            v0 = v0 / d;
            v1 = v1 / d;
            if (v1 < 0) v0 = -2 - v0;
            vs[i * RIE_LANES] = v0;
        }
        for (int i = 1; i < m; ++i) {
            if (vs[(i - 1) * RIE_LANES] > vs[i * RIE_LANES]) {
                const float temp = vs[i * RIE_LANES], tx = px[i * RIE_LANES], ty = py[i * RIE_LANES];
                int j = i;
                while (j > 0 && vs[(j - 1) * RIE_LANES] > temp) {
                    vs[j * RIE_LANES] = vs[(j - 1) * RIE_LANES];
                    px[j * RIE_LANES] = px[(j - 1) * RIE_LANES];
                    py[j * RIE_LANES] = py[(j - 1) * RIE_LANES];
                    --j;
                }
                vs[j * RIE_LANES] = temp; px[j * RIE_LANES] = tx; py[j * RIE_LANES] = ty;
            }
        }
        const float ax = px[0], ay = py[0];
        for (int i = 0; i < m - 2; ++i) {
            const float bx = px[(i + 1) * RIE_LANES], by = py[(i + 1) * RIE_LANES], qx = px[(i + 2) * RIE_LANES], qy = py[(i + 2) * RIE_LANES];
            ai += fabsf(((ax - qx) * (by - qy) - (ay - qy) * (bx - qx)) / 2.0f);
        }
    }
    const float a1 = r1[2] * r1[3], a2 = r2[2] * r2[3];
    if (criterion == -1) return ai / (a1 + a2 - ai);
    if (criterion == 0) return ai / a1;
    if (criterion == 1) return ai / a2;
    return ai;
}

}  // namespace md
