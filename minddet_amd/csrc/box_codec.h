// box_codec.h -- the per-box device arithmetic that more than one translation unit runs: second_box_decode and the standup box.
// detops.hip (md_second_box_decode, md_standup_boxes) and pphead.hip (md_pp_decode_selected) call these two functions and nothing
// else for that arithmetic, so the fused PointPillars decode agrees with the stand-alone operators bit for bit.
#pragma once
#include <hip/hip_runtime.h>

// every product below is rounded before it is added (no fused multiply-add), as in detops.hip: part of the arithmetic both units share
#pragma clang fp contract(off)

namespace md {

// second_box_decode, the non-vector angle form (pointpillars/src/core/box_ops.py:47-85): t = the 7 encodings, a = the anchor
// (x, y, z, w, l, h, r), o = the box (x, y, z, w, l, h, r)
__device__ __forceinline__ void second_box_decode_one(const float *t, const float *a, float *o) {
    const float xa = a[0], ya = a[1], wa = a[3], la = a[4], ha = a[5], ra = a[6];
    const float za = a[2] + ha / 2;
    const float diagonal = sqrtf(la * la + wa * wa);
    const float xg = t[0] * diagonal + xa, yg = t[1] * diagonal + ya, zg = t[2] * ha + za;
    const float lg = expf(t[4]) * la, wg = expf(t[3]) * wa, hg = expf(t[5]) * ha;
    const float rg = t[6] + ra;
    o[0] = xg; o[1] = yg; o[2] = zg - hg / 2; o[3] = wg; o[4] = lg; o[5] = hg; o[6] = rg;
}

// rotated BEV box (x, y, dx, dy, r) -> axis-aligned "standup" box of its 4 corners:
// pointpillars/src/core/box_np_ops.py:316-341 (center_to_corner_box2d, origin 0.5, corners @ [[c,-s],[s,c]])
// + :172-177 (corner_to_standup_nd); call site pointpillars/src/predict.py:61-78.
__device__ __forceinline__ float4 standup_one(float cx, float cy, float dx, float dy, float r) {
    const float s = sinf(r), c = cosf(r);
    const float nx[4] = {-0.5f, -0.5f, 0.5f, 0.5f}, ny[4] = {-0.5f, 0.5f, 0.5f, -0.5f};
    float x0 = 0, x1 = 0, y0 = 0, y1 = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float px = dx * nx[k], py = dy * ny[k];
        const float qx = px * c + py * s + cx, qy = -px * s + py * c + cy;
        if (k == 0) { x0 = x1 = qx; y0 = y1 = qy; }
        else { x0 = fminf(x0, qx); x1 = fmaxf(x1, qx); y0 = fminf(y0, qy); y1 = fmaxf(y1, qy); }
    }
    return make_float4(x0, y0, x1, y1);
}

}  // namespace md
