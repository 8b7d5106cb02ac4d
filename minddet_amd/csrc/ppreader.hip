// ppreader.hip -- the front end of the anchor-based (KITTI) PointPillars: md_pp_pillar_encode (its PillarFeatureNet + PointPillarsScatter
// in one launch), md_pp_anchor_mask (the anchor mask of a whole batch, voxel_num read on the device) and md_anchor_mask (of one sample).  The ABI, the exact semantics
// and the reference lines are in include/minddet_hip_ppreader.h.
//
// md_pp_pillar_encode: one wave owns one voxel at a time (grid-stride over the B x max_voxels rows, rows >= voxel_num[b] skipped
// wave-uniformly).  The reference's Dense runs under to_float(float16): fp16 operands, and products of fp16 values are exact in fp32, so
// the [32 points x K features] x [K x 64] product of a voxel is two v_mfma_f32_32x32x16_f16 with exactly the reference's operand
// precision (K = 10 or 11 of the 16 k slots; the rest are zero).
//   A[point][k]    lane l holds point l & 31, features 8 (l >> 5) .. + 7: each lane loads its point as one float4 straight from global
//                  memory and decorates it in registers; rows >= num_points are zero, so the MFMA itself gives the padded rows' d = 0
//   B[k][channel]  the fp16 weight of channel 32 q + (l & 31), k = 8 (l >> 5) .. + 7, for the two channel halves q: 8 VGPRs, loaded
//                  once per launch
//   C/D            channel on the lane (col = l & 31), the 16 registers are the point rows (reg & 3) + 8 (reg >> 2) + 4 (l >> 5): scale
//                  and shift are per-lane scalars and the maximum over the points is a maximum over registers plus one __shfl_xor(32)
// Every step after the product -- round to fp16, the affine (one fp32 FMA), round to fp16, ReLU -- is monotone in d, rising where
// scale >= 0 and falling where scale < 0.  So the maximum over the rows of the chain equals the chain of the rows' largest (smallest) d,
// bit for bit: the epilogue takes the maximum and the minimum of the 16 registers and runs the chain once per channel.
// The next voxel's row (count, coors, the lane's point) is loaded before the current one is computed: one wave's voxels are a serial
// chain of dependent loads otherwise.  No LDS.
// Sizing (Car config, B = 4: 160 000 rows of 32 x 4 fp32, a 496 x 432 x 64 bf16 canvas): 110 MB of zero fill + 512 B per live row;
// the MFMA work is 2 x 160 000 instructions of 16 passes, under 10 us over 1024 SIMDs.
// DESIGN 9 item 9 has the measured figure (98 us at 40 000 live rows per sample: far from that floor, and not bound by the product).
//
// md_pp_anchor_mask, md_anchor_mask (pointpillars/src/data/preprocess.py:211-225 + core/box_np_ops.py:745-776): four steps (zero,
// scatter-add, cumsum along y and x, 4-corner box sums), each as one launch over the batch; a sample's rows are cut at voxel_num[b] on
// the device.  md_anchor_mask, the mask of one sample from [V, 3] coordinates, is the same launches with B = 1 and no voxel_num.
// Integer counts: the result is exact whatever the atomics' order.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/minddet_hip_ppreader.h"
#include "aot.h"
#include "device.h"
#include "workgroup.h"

namespace md {

constexpr int PR_WAVES = 4;   // waves per workgroup

struct PPEncArgs {
    const float *voxels;     // [B, MV, MP, 4]
    const int *num_points;   // [B, MV]
    const int *coors;        // [B, MV, 4]
    const int *voxel_num;    // [B]
    const float *w;          // [64, K]
    const float *scale, *shift;   // [64]
    uint16_t *canvas;        // [B, H, W, 64]
    int B, MV, MP, H, W, K;
    float vx, vy, vz, x_off, y_off, z_off;
};

// what a wave needs of one voxel row, fetched one voxel ahead
struct PPRow {
    int n;          // num_points, unclamped
    int4 co;        // (b, z, y, x)
    float4 p;       // the lane's point (row lane & 31; zero for rows >= MP)
    bool live;      // v < B * MV and its row < voxel_num[b]
};

__device__ __forceinline__ PPRow pp_fetch(const PPEncArgs &a, int v, int r) {
    PPRow o;
    o.n = 0;
    o.co = make_int4(0, 0, 0, 0);
    o.p = make_float4(0.f, 0.f, 0.f, 0.f);
    o.live = false;
    if (v < a.B * a.MV) {
        const int bv = v / a.MV;
        o.live = v - bv * a.MV < a.voxel_num[bv];                                        // wave-uniform
        if (o.live) {
            o.n = a.num_points[v];
            o.co = *reinterpret_cast<const int4 *>(a.coors + (size_t)v * 4);
            if (r < a.MP) o.p = *reinterpret_cast<const float4 *>(a.voxels + ((size_t)v * a.MP + r) * 4);
        }
    }
    return o;
}

// the chain after the Dense: fp16(d) -> fp16(scale * d + shift) in fp32 -> ReLU; every step monotone in d
__device__ __forceinline__ float pp_chain(float d, float scale, float shift) {
    const float d16 = (float)(_Float16)d;
    const float y16 = (float)(_Float16)fmaf(scale, d16, shift);
    return fmaxf(y16, 0.f);
}

// FULL: MP == 32, every row of the tile is a row of the voxel
template <bool FULL>
__global__ __launch_bounds__(PR_WAVES * 64) void pp_pillar_encode_kernel(PPEncArgs a) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int r = lane & 31, h = lane >> 5;

    // B operand: element j of lane (r, h) is B[k = 8 h + j][col = r] = fp16(w[32 q + r][8 h + j]), zero for k >= K
    f16x8 wb[2];
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int k = 8 * h + j;
            wb[q][j] = (_Float16)(k < a.K ? a.w[(32 * q + r) * a.K + k] : 0.f);
        }
    // the channel this lane finishes and stores: lane = channel (half h of the wave takes channel half q = h)
    const float scale = a.scale[lane], shift = a.shift[lane];
    const bool with_dist = a.K == 11;

    const int wave = blockIdx.x * PR_WAVES + wv, nwaves = gridDim.x * PR_WAVES;
    const int total = a.B * a.MV;
    PPRow next = pp_fetch(a, wave, r);
    for (int v = wave; v < total; v += nwaves) {
        const PPRow cur = next;
        next = pp_fetch(a, v + nwaves, r);
        if (!cur.live) continue;                                                          // wave-uniform
        const int cb = cur.co.x, cz = cur.co.y, cy = cur.co.z, cx = cur.co.w;
        if (cb < 0 || cb >= a.B || cy < 0 || cy >= a.H || cx < 0 || cx >= a.W) continue;
        int n = cur.n;
        n = n < 0 ? 0 : (n > a.MP ? a.MP : n);
        n = __builtin_amdgcn_readfirstlane(n);
        const float4 p = cur.p;

        // mean over the voxel's points: the fp32 sum in row order, then one correctly rounded divide by max(n, 1)
        float sx = 0.f, sy = 0.f, sz = 0.f;
#pragma unroll 1
        for (int i = 0; i < n; ++i) {
            sx = __fadd_rn(sx, __int_as_float(__builtin_amdgcn_readlane(__float_as_int(p.x), i)));
            sy = __fadd_rn(sy, __int_as_float(__builtin_amdgcn_readlane(__float_as_int(p.y), i)));
            sz = __fadd_rn(sz, __int_as_float(__builtin_amdgcn_readlane(__float_as_int(p.z), i)));
        }
        const float fn = (float)(n > 1 ? n : 1);
        const float mx = __fdiv_rn(sx, fn), my = __fdiv_rn(sy, fn), mz = __fdiv_rn(sz, fn);
        const float ctr_x = __fadd_rn(__fmul_rn((float)cx, a.vx), a.x_off);
        const float ctr_y = __fadd_rn(__fmul_rn((float)cy, a.vy), a.y_off);
        const float ctr_z = __fadd_rn(__fmul_rn((float)cz, a.vz), a.z_off);

        // the lane's 8 of the 16 k slots: half 0 holds features 0 .. 7, half 1 features 8, 9 (, 10) and zeros
        float f[8];
        if (h == 0) {
            f[0] = p.x; f[1] = p.y; f[2] = p.z; f[3] = p.w;
            f[4] = __fsub_rn(p.x, mx); f[5] = __fsub_rn(p.y, my); f[6] = __fsub_rn(p.z, mz);
            f[7] = __fsub_rn(p.x, ctr_x);
        } else {
            f[0] = __fsub_rn(p.y, ctr_y);
            f[1] = __fsub_rn(p.z, ctr_z);
            f[2] = with_dist ? __fsqrt_rn(__fadd_rn(__fadd_rn(__fmul_rn(p.x, p.x), __fmul_rn(p.y, p.y)), __fmul_rn(p.z, p.z))) : 0.f;
            f[3] = f[4] = f[5] = f[6] = f[7] = 0.f;
        }
        const bool row_live = r < n;                                                      // the padding mask: rows >= n are zero
        f16x8 av;
#pragma unroll
        for (int j = 0; j < 8; ++j) av[j] = (_Float16)(row_live ? f[j] : 0.f);

        f32x16 acc0 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        f32x16 acc1 = acc0;
        acc0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(av, wb[0], acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(av, wb[1], acc1, 0, 0, 0);

        // largest and smallest d over the voxel's MP rows, per channel: registers, then the other half of the wave
        float hi0 = -INFINITY, lo0 = INFINITY, hi1 = -INFINITY, lo1 = INFINITY;
#pragma unroll
        for (int g = 0; g < 16; ++g) {
            const int row = (g & 3) + 8 * (g >> 2) + 4 * h;
            if (FULL || row < a.MP) {
                hi0 = fmaxf(hi0, acc0[g]); lo0 = fminf(lo0, acc0[g]);
                hi1 = fmaxf(hi1, acc1[g]); lo1 = fminf(lo1, acc1[g]);
            }
        }
        hi0 = fmaxf(hi0, __shfl_xor(hi0, 32, 64)); lo0 = fminf(lo0, __shfl_xor(lo0, 32, 64));
        hi1 = fmaxf(hi1, __shfl_xor(hi1, 32, 64)); lo1 = fminf(lo1, __shfl_xor(lo1, 32, 64));
        // half 0 finishes channels 0 .. 31 of the first MFMA, half 1 channels 32 .. 63 of the second: one 128-byte row
        const float hi = h ? hi1 : hi0, lo = h ? lo1 : lo0;
        const float best = pp_chain(scale >= 0.f ? hi : lo, scale, shift);
        a.canvas[(((size_t)cb * a.H + cy) * a.W + cx) * 64 + lane] = f2bf(best);
    }
}

// ---- the anchor mask of B samples (md_anchor_mask: B = 1): dense count map -> integral image -> 4-corner box sums, integer exact
// coors: B * MV rows of `row` ints with y and x in columns cy and cx; voxel_num: rows of a sample that count, or NULL for all MV
__global__ void amask_scatter_kernel(const int *__restrict__ coors, int row, int cy, int cx, const int *__restrict__ voxel_num, int B,
                                     int MV, int nx, int ny, int *__restrict__ dense) {
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < (size_t)B * MV; e += (size_t)gridDim.x * blockDim.x) {
        const int b = (int)(e / MV), i = (int)(e - (size_t)b * MV);
        if (voxel_num && i >= voxel_num[b]) continue;
        const int y = coors[e * row + cy], x = coors[e * row + cx];
        if ((unsigned)y < (unsigned)ny && (unsigned)x < (unsigned)nx) atomicAdd(&dense[((size_t)b * ny + y) * nx + x], 1);
    }
}
// cumsum along y then along x: one thread per column, one wave per row (maps are ~500 x 500)
__global__ void amask_cumsum_y_kernel(int *__restrict__ dense, int B, int nx, int ny) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= B * nx) return;
    const int b = t / nx, x = t - b * nx;
    int *d = dense + (size_t)b * ny * nx + x;   // the column, one row further each step
    int acc = 0;
    for (int y = 0; y < ny; ++y, d += nx) { acc += d[0]; d[0] = acc; }
}
__global__ void amask_cumsum_x_kernel(int *__restrict__ dense, int B, int nx, int ny) {   // 64-wide chunks with a carry
    const int row = blockIdx.x * (blockDim.x / 64) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= B * ny) return;
    int *d = dense + (size_t)row * nx;
    int carry = 0;
    for (int x0 = 0; x0 < nx; x0 += 64) {
        const int x = x0 + lane;
        const int v = wave_inclusive_scan(x < nx ? d[x] : 0) + carry;
        if (x < nx) d[x] = v;
        carry = __shfl(v, 63, 64);
    }
}
__global__ void amask_area_kernel(const int *__restrict__ dense, const float *__restrict__ bv, int B, int n, int nx, int ny, float sx,
                                  float sy, float ox, float oy, float thr, float *__restrict__ area, unsigned char *__restrict__ mask) {
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < (size_t)B * n; e += (size_t)gridDim.x * blockDim.x) {
        const int s = (int)(e / n), i = (int)(e - (size_t)s * n);
        const int *d = dense + (size_t)s * ny * nx;
        const float4 b = *reinterpret_cast<const float4 *>(bv + (size_t)i * 4);
        int c0 = (int)floorf((b.x - ox) / sx), c1 = (int)floorf((b.y - oy) / sy);
        int c2 = (int)floorf((b.z - ox) / sx), c3 = (int)floorf((b.w - oy) / sy);
        c0 = max(c0, 0); c1 = max(c1, 0); c2 = min(c2, nx - 1); c3 = min(c3, ny - 1);
        // numpy negative indices wrap (a box entirely left of / below the grid): mirror that
        const int C0 = c0, C1 = c1, C2 = c2 < 0 ? c2 + nx : c2, C3 = c3 < 0 ? c3 + ny : c3;
        const int c0w = min(C0, nx - 1), c1w = min(C1, ny - 1);
        const int v = d[C3 * nx + C2] - d[C3 * nx + c0w] - d[c1w * nx + C2] + d[c1w * nx + c0w];
        const float ar = (float)v;
        if (area) area[e] = ar;
        mask[e] = ar > thr ? 1 : 0;
    }
}

// the four steps on `dense` (B ny nx ints).  cap: most workgroups of the two grid-stride launches (md_anchor_mask's grids have no cap)
static int anchor_mask_launch(hipStream_t s, int *dense, const int *coors, int row, int cy, int cx, const int *voxel_num, int64_t B,
                              int64_t MV, const float *bv, int64_t n, const md_anchor_mask_attrs *at, float *area, unsigned char *mask,
                              size_t cap) {
    const int nx = at->grid_x, ny = at->grid_y;
    MD_HIP_TRY(hipMemsetAsync(dense, 0, (size_t)B * ny * nx * 4, s));
    if (MV > 0)
        hipLaunchKernelGGL(amask_scatter_kernel, dim3(grid1d((size_t)(B * MV), cap)), dim3(256), 0, s, coors, row, cy, cx, voxel_num, (int)B,
                           (int)MV, nx, ny, dense);
    hipLaunchKernelGGL(amask_cumsum_y_kernel, dim3((unsigned)((B * nx + 255) / 256)), dim3(256), 0, s, dense, (int)B, nx, ny);
    hipLaunchKernelGGL(amask_cumsum_x_kernel, dim3((unsigned)((B * ny + 3) / 4)), dim3(256), 0, s, dense, (int)B, nx, ny);
    if (n > 0)
        hipLaunchKernelGGL(amask_area_kernel, dim3(grid1d((size_t)(B * n), cap)), dim3(256), 0, s, (const int *)dense, bv, (int)B, (int)n, nx,
                           ny, at->voxel_x, at->voxel_y, at->offset_x, at->offset_y, at->area_threshold, area, mask);
    return launched();
}

static inline bool pr_finite(float x) { return x == x && x - x == 0.f; }

}  // namespace md

using namespace md;

// in : voxels[B,MV,MP,4] f32, num_points[B,MV] i32, coors[B,MV,4] i32, voxel_num[B] i32, w[64,K] f32, scale[64] f32, shift[64] f32 ;
// out: canvas[B,H,W,64] bf16.  extra: md_pp_pillar_encode_attrs (required).  Every check precedes the first device call.
extern "C" int md_pp_pillar_encode(MD_AOT_ARGS) {
    Args g(MD_ARGS, 8, 8);
    const md_pp_pillar_encode_attrs *at = g.attrs<md_pp_pillar_encode_attrs>(extra);
    g.tensor(0, F32, 4); g.tensor(1, I32, 2); g.tensor(2, I32, 3); g.tensor(3, I32, 1); g.tensor(4, F32, 2); g.tensor(5, F32, 1);
    g.tensor(6, F32, 1); g.tensor(7, BF16, 4);
    if (int rc = g.rc()) return rc;
    if (at->reserved0 != 0 || (at->with_distance != 0 && at->with_distance != 1)) return MD_ERR_ARG;
    for (float v : {at->vx, at->vy, at->vz})
        if (!pr_finite(v) || !(v > 0.f)) return MD_ERR_ARG;
    for (float v : {at->x_offset, at->y_offset, at->z_offset})
        if (!pr_finite(v)) return MD_ERR_ARG;
    const int64_t B = g.d(0, 0), MV = g.d(0, 1), MP = g.d(0, 2), F = g.d(0, 3), K = g.d(4, 1);
    const int64_t H = g.d(7, 1), W = g.d(7, 2);
    if (F != 4 || K != 10 + at->with_distance) return MD_ERR_ARG;
    if (g.d(1, 0) != B || g.d(1, 1) != MV || g.d(2, 0) != B || g.d(2, 1) != MV || g.d(2, 2) != 4 || g.d(3, 0) != B) return MD_ERR_ARG;
    if (g.d(4, 0) != 64 || g.d(5, 0) != 64 || g.d(6, 0) != 64) return MD_ERR_ARG;
    if (g.d(7, 0) != B || g.d(7, 3) != 64 || H < 0 || W < 0 || B < 0 || MV < 0 || MP < 0) return MD_ERR_ARG;
    if (MP > 32) return MD_ERR_SIZE;
    if (mul({B, MV}) >= (1 << 30) || !fits_i32(mul({B, MV, MP})) || H > 65536 || W > 65536 || !fits_i32(mul({B, H, W}) / 4))
        return MD_ERR_SIZE;
    if (B * H * W == 0) return MD_OK;
    if (!g.have({0, 1, 2, 3, 4, 5, 6, 7})) return MD_ERR_ARG;
    PPEncArgs a;
    a.voxels = g.ptr<const float>(0); a.num_points = g.ptr<const int>(1); a.coors = g.ptr<const int>(2); a.voxel_num = g.ptr<const int>(3);
    a.w = g.ptr<const float>(4); a.scale = g.ptr<const float>(5); a.shift = g.ptr<const float>(6);
    a.canvas = g.ptr<uint16_t>(7);
    a.B = (int)B; a.MV = (int)MV; a.MP = (int)MP; a.H = (int)H; a.W = (int)W; a.K = (int)K;
    a.vx = at->vx; a.vy = at->vy; a.vz = at->vz; a.x_off = at->x_offset; a.y_off = at->y_offset; a.z_off = at->z_offset;
    hipStream_t s = (hipStream_t)stream;
    MD_HIP_TRY(hipMemsetAsync(a.canvas, 0, (size_t)(B * H * W) * 64 * 2, s));   // cells without a pillar are zero
    if (B * MV == 0 || MP == 0) return MD_OK;
    const size_t wgs = (size_t)(B * MV + PR_WAVES - 1) / PR_WAVES;
    hipLaunchKernelGGL(MP == 32 ? pp_pillar_encode_kernel<true> : pp_pillar_encode_kernel<false>, dim3((unsigned)(wgs < 2048 ? wgs : 2048)),
                       dim3(PR_WAVES * 64), 0, s, a);
    return launched();
}

// scratch of md_pp_anchor_mask: one i32 per cell of every sample's grid, [B][grid_y][grid_x]
extern "C" int64_t md_pp_anchor_mask_workspace_bytes(int64_t B, int64_t grid_x, int64_t grid_y) {
    return any_negative({B, grid_x, grid_y}) ? -1 : ws_answer((int64_t)(Sz(B) * grid_y * grid_x * 4));
}

// in : coors[B,MV,4] i32, voxel_num[B] i32, anchors_bv[N,4] f32 ; out: mask[B,N] u8 [, area[B,N] f32 or NULL] [, workspace u8].
// extra: md_anchor_mask_attrs (required).
extern "C" int md_pp_anchor_mask(MD_AOT_ARGS) {
    Args g(MD_ARGS, 4, 6);
    const md_anchor_mask_attrs *at = g.attrs<md_anchor_mask_attrs>(extra);
    g.tensor(0, I32, 3); g.tensor(1, I32, 1); g.tensor(2, F32, 2); g.tensor(3, U8, 2); g.optional(4, F32, 2);
    if (int rc = g.rc()) return rc;
    const int64_t B = g.d(0, 0), MV = g.d(0, 1), n = g.d(2, 0);
    if (B < 0 || MV < 0 || n < 0 || g.d(0, 2) != 4 || g.d(1, 0) != B || g.d(2, 1) != 4 || g.d(3, 0) != B || g.d(3, 1) != n) return MD_ERR_ARG;
    if (g.given(4) && (g.d(4, 0) != B || g.d(4, 1) != n)) return MD_ERR_ARG;
    const int nx = at->grid_x, ny = at->grid_y;
    if (nx < 1 || ny < 1 || mul({nx, ny, B > 0 ? B : 1}) > (1 << 28)) return MD_ERR_SIZE;
    if (!fits_i32(mul({B, n})) || !fits_i32(mul({B, MV}))) return MD_ERR_SIZE;
    if (B == 0) return MD_OK;
    if ((MV > 0 && !g.have({0})) || !g.have({1}) || (n > 0 && !g.have({2, 3}))) return MD_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    Scratch ws;
    if (int rc = ws.acquire((size_t)md_pp_anchor_mask_workspace_bytes(B, nx, ny), g, 5, s)) return rc;
    return anchor_mask_launch(s, (int *)ws.ptr, g.ptr<const int>(0), 4, 2, 3, g.ptr<const int>(1), B, MV, g.ptr<const float>(2), n, at,
                              g.given(4) ? g.ptr<float>(4) : nullptr, g.ptr<unsigned char>(3), 16384);
}

// The mask of one sample.  in: coors[V,3] i32 (z,y,x), anchors_bv[N,4] f32 ; out: area[N] f32, mask[N] u8 ; ws: ny*nx i32
extern "C" int md_anchor_mask(MD_AOT_ARGS) {
    Args a(MD_ARGS, 4, 5);
    const md_anchor_mask_attrs *at = a.attrs<md_anchor_mask_attrs>(extra);
    a.tensor(0, I32, 2); a.tensor(1, F32, 2); a.tensor(2, F32); a.tensor(3, U8);
    const int64_t nv = a.d(0, 0), n = a.d(1, 0);
    a.require(nv >= 0 && n >= 0 && a.d(0, 1) == 3 && a.d(1, 1) == 4 && a.numel(2) >= n && a.numel(3) >= n);
    if (int rc = a.rc()) return rc;
    const int nx = at->grid_x, ny = at->grid_y;
    if (nx < 1 || ny < 1 || (int64_t)nx * ny > (1 << 28)) return MD_ERR_SIZE;
    if ((nv > 0 && !a.have({0})) || (n > 0 && !a.have({1, 2, 3}))) return MD_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    Scratch ws;
    if (int rc = ws.acquire((size_t)nx * ny * 4, a, 4, s)) return rc;
    return anchor_mask_launch(s, (int *)ws.ptr, (const int *)params[0], 3, 1, 2, nullptr, 1, nv, (const float *)params[1], n, at,
                              (float *)params[2], (unsigned char *)params[3], ~(size_t)0);
}
