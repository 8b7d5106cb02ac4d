// box_codec.h -- the per-box device arithmetic that more than one translation unit runs: second_box_decode, the standup box and the
// delta-to-box decode.  detops.hip (md_second_box_decode, md_standup_boxes) and pphead.hip (md_pp_decode_selected) call the first two
// and nothing else for that arithmetic, so the fused PointPillars decode agrees with the stand-alone operators bit for bit;
// detops.hip (md_delta2bbox) and twostage.hip (the RPN and R-CNN decodes) call the third.  The CenterPoint cell arithmetic
// (cp_score_one, cp_box_one) is shared the same way by detops.hip (md_centerpoint_decode) and cphead.hip (md_cp_scores,
// md_cp_decode_selected).
#pragma once
#include <hip/hip_runtime.h>
#include <float.h>
#include <stdint.h>

#include "device.h"

namespace md {

// delta2bbox (the public mmdet definition): deltas (dx, dy, dw, dh), denormalised by p.mean / p.stdv, applied to the box r = (x1, y1, x2,
// y2); dw, dh clamped to +-p.max_ratio.  clip_box then clamps the result to [0, w] x [0, h]; WHETHER to clip is the caller's decision and
// stays at the call: md_delta2bbox clips when clip_w > 0 && clip_h > 0 (its do_clip), the two-stage decodes when p.clip_w > 0.
// These two functions stand ABOVE the contraction pragma below and so takes the mode of the unit that includes it: detops.hip switches
// contraction off first (every product rounded, as its float64-judged contract says), twostage.hip keeps the compiler's fused
// multiply-adds.  Both are what the two units computed when each had its own copy.
struct DecodeP { float mean[4], stdv[4]; float max_ratio, clip_w, clip_h; };
__device__ __forceinline__ float4 delta2bbox_one(float4 r, float dx, float dy, float dw, float dh, const DecodeP &p) {
    dx = dx * p.stdv[0] + p.mean[0]; dy = dy * p.stdv[1] + p.mean[1];
    dw = dw * p.stdv[2] + p.mean[2]; dh = dh * p.stdv[3] + p.mean[3];
    dw = fminf(fmaxf(dw, -p.max_ratio), p.max_ratio);
    dh = fminf(fmaxf(dh, -p.max_ratio), p.max_ratio);
    const float px = (r.x + r.z) * 0.5f, py = (r.y + r.w) * 0.5f, pw = r.z - r.x, ph = r.w - r.y;
    const float gw = pw * expf(dw), gh = ph * expf(dh);
    const float gx = px + pw * dx, gy = py + ph * dy;
    return make_float4(gx - gw * 0.5f, gy - gh * 0.5f, gx + gw * 0.5f, gy + gh * 0.5f);
}
__device__ __forceinline__ float4 clip_box(float4 b, float w, float h) {
    const float x1 = fminf(fmaxf(b.x, 0.f), w), x2 = fminf(fmaxf(b.z, 0.f), w);
    const float y1 = fminf(fmaxf(b.y, 0.f), h), y2 = fminf(fmaxf(b.w, 0.f), h);
    return make_float4(x1, y1, x2, y2);
}

}  // namespace md

// every product below is rounded before it is added (no fused multiply-add), as in detops.hip: part of the arithmetic the units share
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

// CenterPoint head, one BEV cell of one task (center_head.py:297-334 predict, :408-423 the score / range mask).  h: the cell's
// channels (bf16 bits; global memory or LDS), t: the task's first channels, g: the geometry of the test config.
struct CpTask { int o_reg, o_height, o_dim, o_rot, o_vel, o_hm, ncls; };
struct CpGeom { float score_thr, osf, vx, vy, px, py; float rmin[3], rmax[3]; };

// -> the cell's score: the first maximum of sigmoid(hm_c) where it is > score_thr and the centre lies inside post_center_range, else
// -1.  lab = the class of that maximum (whatever the mask says), c = the centre (xs, ys, zs).
__device__ __forceinline__ float cp_score_one(const uint16_t *h, const CpTask &t, const CpGeom &g, int x, int y, int &lab, float *c) {
    float best = -FLT_MAX;
    lab = 0;
    for (int k = 0; k < t.ncls; ++k) {  // ArgMaxWithValue: first maximum wins
        const float v = sigmoid(bf2f(h[t.o_hm + k]));
        if (v > best) { best = v; lab = k; }
    }
    const float xs = ((float)x + bf2f(h[t.o_reg])) * g.osf * g.vx + g.px;
    const float ys = ((float)y + bf2f(h[t.o_reg + 1])) * g.osf * g.vy + g.py;
    const float zs = bf2f(h[t.o_height]);
    const bool in_range = xs >= g.rmin[0] && ys >= g.rmin[1] && zs >= g.rmin[2] && xs <= g.rmax[0] && ys <= g.rmax[1] && zs <= g.rmax[2];
    const bool ok = best > g.score_thr && in_range;
    c[0] = xs; c[1] = ys; c[2] = zs;
    return ok ? best : -1.f;
}

// the box of a cell that passed the mask: b = (x, y, z, dx, dy, dz, vx, vy, rot), nb = the NMS operand (x, y, z, dy, dx, dz,
// -rot - pi/2: center_head.py:426-430)
__device__ __forceinline__ void cp_box_one(const uint16_t *h, const CpTask &t, const float *c, float *b, float *nb) {
    const float d0 = expf(bf2f(h[t.o_dim])), d1 = expf(bf2f(h[t.o_dim + 1])), d2 = expf(bf2f(h[t.o_dim + 2]));
    const float rot = atan2f(bf2f(h[t.o_rot]), bf2f(h[t.o_rot + 1]));
    const float v0 = t.o_vel >= 0 ? bf2f(h[t.o_vel]) : 0.f, v1 = t.o_vel >= 0 ? bf2f(h[t.o_vel + 1]) : 0.f;
    b[0] = c[0]; b[1] = c[1]; b[2] = c[2]; b[3] = d0; b[4] = d1; b[5] = d2; b[6] = v0; b[7] = v1; b[8] = rot;
    const float r2 = -rot - 1.5707963267948966f;
    nb[0] = c[0]; nb[1] = c[1]; nb[2] = c[2]; nb[3] = d1; nb[4] = d0; nb[5] = d2; nb[6] = r2;
}

}  // namespace md
