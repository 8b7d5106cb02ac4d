// cntargets.hip -- CenterNet training targets on the device (include/minddet_hip_cn.h; cnloss.hip consumes the outputs).
//
// What it replaces: the target part of COCOHP.preprocess_fn (minddet/models/centernet/src/dataset.py:317-384) with gaussian_radius /
// gaussian2D / draw_umich_gaussian (src/image.py:94-144): a Python loop per object with a numpy window maximum per Gaussian, on the host.
// Two launches, no memset, no atomics, no host read:
//   cn_row_kernel   one lane per (sample, slot): clip, size test, radius, centre; wh / ind / reg / reg_mask written for every slot (zeros
//                   for a skipped row and for the slots past G) and the draw list (ct_int x, y, radius, class; radius -1 = nothing
//                   to draw) left in the workspace, one entry per slot
//   cn_heat_kernel  heatmap.h's heat_tile on one 64 x 16 tile of one (sample, class) map, the sample's draw list filtered by class.  A
//                   map no object of its class touches costs the list scan per workgroup and the zero fill, nothing per cell.
// The fp32 steps in the operation order of the numpy code under NumPy >= 2 scalar promotion (fp contraction off); radius and Gaussian
// in float64.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "aot.h"
#include "../../include/minddet_hip_cn.h"

#pragma clang fp contract(off)

#include "heatmap.h"

namespace md {

static_assert(sizeof(md_cn_targets_attrs) == 4, "minddet_hip_cn.h: attribute struct layout");

constexpr int CNT_MAX_M = MD_CN_MAX_OBJS;

struct CntParams {
    int B, G, M, C, H, W;
    double overlap;
};

// gaussian_radius((height, width), min_overlap), image.py:94-114 term by term in float64 on two integers
__device__ __forceinline__ double gaussian_radius_f64(int height, int width, double o) {
    const double hw = (double)(height + width), wh = (double)(width * height);
    const double b1 = hw;
    const double c1 = wh * (1.0 - o) / (1.0 + o);
    const double sq1 = sqrt(b1 * b1 - 4.0 * c1);
    const double r1 = (b1 + sq1) / 2.0;
    const double b2 = 2.0 * hw;
    const double c2 = (1.0 - o) * (double)width * (double)height;
    const double sq2 = sqrt(b2 * b2 - 16.0 * c2);
    const double r2 = (b2 + sq2) / 2.0;
    const double a3 = 4.0 * o;
    const double b3 = -2.0 * o * hw;
    const double c3 = (o - 1.0) * (double)width * (double)height;
    const double sq3 = sqrt(b3 * b3 - 4.0 * a3 * c3);
    const double r3 = (b3 + sq3) / 2.0;
    return fmin(fmin(r1, r2), r3);
}

// np.clip in fp32: a NaN stays a NaN (fminf / fmaxf would drop it)
__device__ __forceinline__ float clip_keep_nan(float v, float hi) { return v < 0.f ? 0.f : (v > hi ? hi : v); }

__global__ __launch_bounds__(256) void cn_row_kernel(const float *__restrict__ boxes, const int *__restrict__ classes, CntParams p,
                                                     int *__restrict__ ind, uint8_t *__restrict__ mask, float *__restrict__ wh,
                                                     float *__restrict__ reg, int4 *__restrict__ draw) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= p.B * p.M) return;
    const int b = e / p.M, k = e - b * p.M;
    float w = 0.f, h = 0.f, rx = 0.f, ry = 0.f;
    int cell = 0, cx = 0, cy = 0, radius = -1, cls = 0;
    if (k < p.G) {
        const float *g = boxes + ((size_t)b * p.G + k) * 4;
        cls = classes[(size_t)b * p.G + k];
        const float x0 = clip_keep_nan(g[0], (float)(p.W - 1)), y0 = clip_keep_nan(g[1], (float)(p.H - 1));
        const float x1 = clip_keep_nan(g[2], (float)(p.W - 1)), y1 = clip_keep_nan(g[3], (float)(p.H - 1));
        const float hh = y1 - y0, ww = x1 - x0;
        if (cls >= 1 && cls <= p.C && hh > 0.f && ww > 0.f) {   // (false for a NaN; the four clipped values are then inside the map)
            const double r = gaussian_radius_f64((int)ceilf(hh), (int)ceilf(ww), p.overlap);
            radius = max(0, (int)fmin(r, 1073741824.0));
            const float ctx = (x0 + x1) / 2.f, cty = (y0 + y1) / 2.f;
            cx = (int)ctx;
            cy = (int)cty;
            w = ww; h = hh;
            rx = ctx - (float)cx; ry = cty - (float)cy;
            cell = cy * p.W + cx;
        }
    }
    const bool used = radius >= 0;
    ind[e] = cell;
    mask[e] = used ? 1 : 0;
    wh[(size_t)e * 2] = w; wh[(size_t)e * 2 + 1] = h;
    reg[(size_t)e * 2] = rx; reg[(size_t)e * 2 + 1] = ry;
    draw[e] = make_int4(cx, cy, radius, used ? cls - 1 : -1);
}

__global__ __launch_bounds__(256) void cn_heat_kernel(const int4 *__restrict__ draw, CntParams p, int tiles_x, float *__restrict__ hm) {
    const int c = blockIdx.y, b = blockIdx.z;
    // (slots past G hold radius -1)
    heat_tile<CNT_MAX_M>(draw + (size_t)b * p.M, min(p.G, p.M), c, blockIdx.x, tiles_x, p.H, p.W, hm + ((size_t)b * p.C + c) * p.H * p.W);
}

}  // namespace md

using namespace md;

// scratch of md_cn_assign_targets: draw[B][M] int4
extern "C" int64_t md_cn_assign_targets_workspace_bytes(int64_t B, int64_t M) {
    return any_negative({B, M}) ? -1 : ws_answer((int64_t)(Sz(B) * M * 16));
}

extern "C" int md_cn_assign_targets(MD_AOT_ARGS) {
    // in : boxes[B,G,4] f32, classes[B,G] i32
    // out: hm[B,C,H,W] f32, ind[B,M] i32, reg_mask[B,M] u8, wh[B,M,2] f32, reg[B,M,2] f32 ; [workspace >= 16 B M bytes]
    Args a(MD_ARGS, 7, 8);
    const md_cn_targets_attrs *at = a.attrs<md_cn_targets_attrs>(extra);
    a.tensor(0, F32, 3); a.tensor(1, I32, 2); a.tensor(2, F32, 4); a.tensor(3, I32, 2); a.tensor(4, U8, 2); a.tensor(5, F32, 3);
    a.tensor(6, F32, 3); a.scratch(7);
    if (int rc = a.rc()) return rc;
    const int64_t B = a.d(0, 0), G = a.d(0, 1), C = a.d(2, 1), H = a.d(2, 2), W = a.d(2, 3), M = a.d(3, 1);
    a.require(B >= 0 && G >= 0 && M >= 0 && C >= 1 && H >= 1 && W >= 1 && a.d(0, 2) == 4 && a.d(1, 0) == B && a.d(1, 1) == G);
    a.require(a.d(2, 0) == B && a.d(3, 0) == B && a.d(4, 0) == B && a.d(4, 1) == M);
    for (int i = 5; i <= 6; ++i) a.require(a.d(i, 0) == B && a.d(i, 1) == M && a.d(i, 2) == 2);
    a.require(G <= M);
    a.require(at->min_overlap > 0.f && at->min_overlap < 1.f);   // (false for a NaN)
    if (int rc = a.rc()) return rc;
    const int64_t lim = (int64_t)1 << 30;
    if (M > CNT_MAX_M || mul({B, G, 4}) >= lim || a.numel(2) >= lim || mul({B, M, 2}) >= lim || B > 65535 || C > 65535) return MD_ERR_SIZE;
    if (B == 0) return MD_OK;
    if (!a.have({0, 1, 2, 3, 4, 5, 6})) return MD_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    Scratch ws;
    if (int rc = ws.acquire((size_t)md_cn_assign_targets_workspace_bytes(B, M), a, 7, s)) return rc;
    if ((uintptr_t)ws.ptr % 16 != 0) return MD_ERR_ARG;
    CntParams p;
    p.B = (int)B; p.G = (int)G; p.M = (int)M; p.C = (int)C; p.H = (int)H; p.W = (int)W;
    p.overlap = (double)at->min_overlap;
    int4 *draw = (int4 *)ws.ptr;
    if (M > 0)
        hipLaunchKernelGGL(cn_row_kernel, dim3((unsigned)((B * M + 255) / 256)), dim3(256), 0, s, (const float *)params[0],
                           (const int *)params[1], p, (int *)params[3], (uint8_t *)params[4], (float *)params[5], (float *)params[6], draw);
    const int tiles_x = (int)((W + HEAT_TILE_W - 1) / HEAT_TILE_W), tiles_y = (int)((H + HEAT_TILE_H - 1) / HEAT_TILE_H);
    hipLaunchKernelGGL(cn_heat_kernel, dim3((unsigned)(tiles_x * tiles_y), (unsigned)C, (unsigned)B), dim3(256), 0, s, draw, p, tiles_x,
                       (float *)params[2]);
    return launched();
}
