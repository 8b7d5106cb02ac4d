// heatmap.h -- the Gaussian heat map of the centre-based training targets (cptargets.hip: CenterPoint, cntargets.hip: CenterNet) in
// gather form, stated once.  A draw-list entry is an int4: centre x, centre y, radius, class; radius -1 means nothing to draw.
// One workgroup of 256 lanes owns one 64 x 16 tile of one (H, W) plane: the list is compacted, in list order, to the entries of the
// plane's class whose window meets the tile; each lane takes the maximum over them for its four consecutive x cells and stores them
// once, zeros included (16-byte stores where the row pitch allows) -- no memset, no atomics.  The Gaussian in float64, fp contraction off.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "workgroup.h"

#pragma clang fp contract(off)

namespace md {

constexpr int HEAT_TILE_W = 64, HEAT_TILE_H = 16;   // 16 lanes x 4 cells wide, 16 rows: one cell quad per lane of a 256-lane workgroup

// CAP: the longest list (static LDS: 32 CAP bytes).  dl[0 .. n): the list; c: the plane's class; tile: its index, tiles_x to a row
template <int CAP>
__device__ __forceinline__ void heat_tile(const int4 *__restrict__ dl, int n, int c, int tile, int tiles_x, int H, int W,
                                          float *__restrict__ plane) {
    __shared__ int4 obj[CAP];        // the surviving entries: (cx, cy, radius, -)
    __shared__ double den[CAP];      // 2 s s of each
    __shared__ int wave_cnt[4];
    __shared__ int n_obj;
    const int tx0 = (tile % tiles_x) * HEAT_TILE_W, ty0 = (tile / tiles_x) * HEAT_TILE_H;
    const int tx1 = min(tx0 + HEAT_TILE_W, W) - 1, ty1 = min(ty0 + HEAT_TILE_H, H) - 1;
    if (threadIdx.x == 0) n_obj = 0;
    __syncthreads();
    for (int j0 = 0; j0 < n; j0 += 256) {
        const int j = j0 + threadIdx.x;
        int4 e = make_int4(0, 0, -1, -1);
        if (j < n) e = dl[j];
        // the window [cx - r, cx + r] x [cy - r, cy + r] meets the tile (written so that no sum can overflow)
        const bool keep = e.z >= 0 && e.w == c && e.z >= tx0 - e.x && e.z >= e.x - tx1 && e.z >= ty0 - e.y && e.z >= e.y - ty1;
        const int at = block_append(keep, wave_cnt, &n_obj);
        if (keep) {
            obj[at] = e;
            const double sigma = (2.0 * (double)e.z + 1.0) / 6.0;   // diameter / 6
            den[at] = 2.0 * sigma * sigma;
        }
        __syncthreads();
        if (threadIdx.x == 0) n_obj += wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
        __syncthreads();
    }
    const int m = n_obj;
    const int y = ty0 + (threadIdx.x >> 4), x0 = tx0 + (threadIdx.x & 15) * 4;
    if (y >= H || x0 >= W) return;
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    for (int o = 0; o < m; ++o) {
        const int4 e = obj[o];
        const int dy = y - e.y;
        if (abs(dy) > e.z) continue;
        const double dy2 = (double)dy * (double)dy, d = den[o];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int dx = x0 + i - e.x;
            if (abs(dx) <= e.z) {
                // gaussian2D's cut h < eps * max can never fire: the smallest value, at a corner, is exp(-2 r r / (2 s s)) with
                // s = (2 r + 1) / 6 > r / 3, which is above exp(-9), far above 2.2e-16
                const float gval = (float)exp(-((double)dx * (double)dx + dy2) / d);
                v[i] = fmaxf(v[i], gval);
            }
        }
    }
    float *dst = plane + (size_t)y * W + x0;
    if (x0 + 3 < W && ((uintptr_t)dst & 15) == 0) {
        *(float4 *)dst = make_float4(v[0], v[1], v[2], v[3]);
    } else {
        for (int i = 0; i < 4 && x0 + i < W; ++i) dst[i] = v[i];
    }
}

}  // namespace md
