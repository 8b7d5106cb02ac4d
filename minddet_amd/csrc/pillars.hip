// pillars.hip -- the point-cloud front end of the pillar detectors: md_voxelize (points -> voxels) and md_pillar_encode (PillarFeatureNet +
// PointPillarsScatter in one launch).  The ABI, the exact semantics and the reference lines are in include/minddet_hip_points.h.
//
// md_voxelize: the reference is a sequential loop over the points (point_cloud_ops.py:5-53); the parallel form computes the same result
// from order-free facts, so it is bit-exact and deterministic whatever the execution order of the atomics:
//   1 cell      per point: its sample b and cell c (fp32 subtract, correctly rounded divide, floor); atomicMin(first[b, c], i)
//   2 flag      a point is the FIRST of its cell iff first[cell] == i; an exclusive prefix sum of the flags over the point index gives
//               every first point the number of voxels the sequential loop had opened before it: its voxel's rank in the sample is
//               pre[i] - pre[offsets[b]].  rank >= max_voxels: the loop dropped that cell with all its points
//   3 count     per kept voxel the number of its points (atomicAdd), an exclusive prefix sum -> CSR offsets, buckets filled through
//               an atomic slot counter (bucket order is arbitrary)
//   4 gather    one wave per voxel: a point's slot is the number of smaller point indices in its bucket (its position in index order);
//               slots < max_points are copied -- the first max_points points by index, in index order
// All atomics are ordinary vector atomics on global memory.  The outputs are zero-filled first, so unused rows and slots are zero.
//
// md_pillar_encode: one wave owns one voxel at a time (grid-stride over the B x max_voxels rows, rows >= voxel_num[b] skipped); lane =
// output channel.  The folded weights of the lane's channel stay in registers for the whole launch; the voxel's points, the first
// layer's rows and the two per-voxel constant rows (the padded row relu(shift), the row maximum) live in a wave-private LDS slab and are
// read as broadcasts (every lane the same address).  Only the rows < num_points are computed: the padded rows are identical, so their
// contribution to the maximum is computed once per voxel.  fp32 FMA throughout; the one bf16 rounding is the final store.
// Sizing (B = 4, 60 000 x 20 rows, two layers): 21 GMAC on dense rows, an HBM floor of 28 us (96 MB voxels + 128 MB canvas at 8 TB/s);
// the launch is bound by the fp32 FMA rate and the LDS broadcasts, not by HBM -- DESIGN 9 has the measured figure.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/minddet_hip_points.h"
#include "aot.h"
#include "device.h"
#include "workgroup.h"

namespace md {

constexpr int PV_THREADS = 256;
constexpr int PV_ITEMS = 4;                       // values per thread of a scan block
constexpr int PV_BLOCK = PV_THREADS * PV_ITEMS;   // values per scan block

struct VoxArgs {
    const float *points;    // [N, F]
    const int *offsets;     // [B + 1]
    float *voxels;          // [B, MV, MP, F]
    int *coors;             // [B, MV, 4]
    int *num_points;        // [B, MV]
    int *voxel_num;         // [B]
    int N, F, B, MV, MP;
    int gx, gy, gz, G;      // cells per axis, cells per sample
    float lo[3], vs[3];
    // workspace
    int *first;             // [B * G]   smallest point index of the cell
    int *cell_vox;          // [B * G]   voxel row (b * MV + rank) of the cell, -1 = dropped; written for every touched cell
    int *cell_of;           // [N]       b * G + cell, -1 = point dropped
    int *flag;              // [N]       1 = first point of its cell; later the buckets
    int *pre;               // [N + 1]   exclusive prefix sum of flag
    int *cnt;               // [B * MV]  points of the voxel
    int *start;             // [B * MV + 1]
    int *bsum;              // block sums of the scans
};

// sample of point i: offsets are device data, so nothing about them is assumed -- a point outside [offsets[0], offsets[B]) has no sample
__device__ __forceinline__ int pv_sample(const int *off, int B, int i) {
    if (i < off[0]) return -1;
    int b = -1;
    for (int k = 0; k < B; ++k)
        if (i >= off[k] && i < off[k + 1]) { b = k; break; }
    return b;
}

__device__ __forceinline__ int pv_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__global__ __launch_bounds__(PV_THREADS) void vox_cell_kernel(VoxArgs a) {
    for (int i = blockIdx.x * PV_THREADS + threadIdx.x; i < a.N; i += gridDim.x * PV_THREADS) {
        const int b = pv_sample(a.offsets, a.B, i);
        int cell = -1;
        if (b >= 0) {
            const float *p = a.points + (size_t)i * a.F;
            // c = floor((p - lo) / vs) in fp32: one rounded subtract, one correctly rounded divide (never a reciprocal multiply)
            const float cx = floorf(__fdiv_rn(__fsub_rn(p[0], a.lo[0]), a.vs[0]));
            const float cy = floorf(__fdiv_rn(__fsub_rn(p[1], a.lo[1]), a.vs[1]));
            const float cz = floorf(__fdiv_rn(__fsub_rn(p[2], a.lo[2]), a.vs[2]));
            // written so that a NaN fails every test
            const bool in = cx >= 0.f && cx < (float)a.gx && cy >= 0.f && cy < (float)a.gy && cz >= 0.f && cz < (float)a.gz;
            if (in) {
                cell = b * a.G + ((int)cz * a.gy + (int)cy) * a.gx + (int)cx;
                atomicMin(&a.first[cell], i);
            }
        }
        a.cell_of[i] = cell;
    }
}

__global__ __launch_bounds__(PV_THREADS) void vox_flag_kernel(VoxArgs a) {
    for (int i = blockIdx.x * PV_THREADS + threadIdx.x; i < a.N; i += gridDim.x * PV_THREADS) {
        const int cell = a.cell_of[i];
        a.flag[i] = cell >= 0 && a.first[cell] == i;
    }
}

// ---- exclusive prefix sum of an int array in three launches: block sums, one workgroup over the block sums, the blocks again
__device__ __forceinline__ int pv_block_exclusive(int v, int *total) {   // exclusive scan of one value per thread over the workgroup
    __shared__ int wsum[PV_THREADS / 64];
    return block_exclusive_scan<PV_THREADS / 64>(v, wsum, *total);   // (its leading barrier: a second call must not overwrite wsum under a reader)
}

__global__ __launch_bounds__(PV_THREADS) void scan_reduce_kernel(const int *val, int n, int *bsum) {
    const int i0 = blockIdx.x * PV_BLOCK + threadIdx.x * PV_ITEMS;
    int s = 0;
#pragma unroll
    for (int k = 0; k < PV_ITEMS; ++k)
        if (i0 + k < n) s += val[i0 + k];
    int total;
    pv_block_exclusive(s, &total);
    if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}

__global__ __launch_bounds__(PV_THREADS) void scan_top_kernel(int *bsum, int nb) {   // one workgroup; bsum -> its exclusive prefix, in place
    __shared__ int wsum[PV_THREADS / 64];
    scan_block_counts<PV_THREADS / 64>(bsum, nb, wsum);
}

__global__ __launch_bounds__(PV_THREADS) void scan_down_kernel(const int *val, int n, const int *bsum, int *out) {   // out[n + 1]
    const int i0 = blockIdx.x * PV_BLOCK + threadIdx.x * PV_ITEMS;
    int v[PV_ITEMS], s = 0;
#pragma unroll
    for (int k = 0; k < PV_ITEMS; ++k) {
        v[k] = i0 + k < n ? val[i0 + k] : 0;
        s += v[k];
    }
    int total;
    int ex = pv_block_exclusive(s, &total) + bsum[blockIdx.x];
#pragma unroll
    for (int k = 0; k < PV_ITEMS; ++k) {
        if (i0 + k < n) out[i0 + k] = ex;
        ex += v[k];
        if (i0 + k == n - 1) out[n] = ex;
    }
}

__global__ __launch_bounds__(PV_THREADS) void vox_rank_kernel(VoxArgs a) {
    const int t = blockIdx.x * PV_THREADS + threadIdx.x;
    for (int b = t; b < a.B; b += gridDim.x * PV_THREADS) {   // voxels the sequential loop opens in sample b
        const int n = a.pre[pv_clamp(a.offsets[b + 1], 0, a.N)] - a.pre[pv_clamp(a.offsets[b], 0, a.N)];
        a.voxel_num[b] = pv_clamp(n, 0, a.MV);
    }
    for (int i = t; i < a.N; i += gridDim.x * PV_THREADS) {
        const int cell = a.cell_of[i];
        if (cell < 0 || a.first[cell] != i) continue;
        const int b = cell / a.G;
        const int rank = a.pre[i] - a.pre[pv_clamp(a.offsets[b], 0, a.N)];   // cells opened before this one, in first-point order
        const bool keep = rank >= 0 && rank < a.MV;
        a.cell_vox[cell] = keep ? b * a.MV + rank : -1;
        if (keep) {
            const int c = cell - b * a.G;
            int *co = a.coors + (size_t)(b * a.MV + rank) * 4;
            co[0] = b;
            co[1] = c / (a.gx * a.gy);
            co[2] = c / a.gx % a.gy;
            co[3] = c % a.gx;
        }
    }
}

__global__ __launch_bounds__(PV_THREADS) void vox_count_kernel(VoxArgs a) {
    for (int i = blockIdx.x * PV_THREADS + threadIdx.x; i < a.N; i += gridDim.x * PV_THREADS) {
        const int cell = a.cell_of[i];
        const int v = cell >= 0 ? a.cell_vox[cell] : -1;
        if (v >= 0) atomicAdd(&a.cnt[v], 1);
    }
}

__global__ __launch_bounds__(PV_THREADS) void vox_fill_kernel(VoxArgs a) {   // cnt counts down to zero: the slot counter of the buckets
    for (int i = blockIdx.x * PV_THREADS + threadIdx.x; i < a.N; i += gridDim.x * PV_THREADS) {
        const int cell = a.cell_of[i];
        const int v = cell >= 0 ? a.cell_vox[cell] : -1;
        if (v >= 0) {
            const int slot = atomicSub(&a.cnt[v], 1) - 1;
            const int at = a.start[v] + slot;
            if (slot >= 0 && at >= 0 && at < a.N) a.flag[at] = i;   // (flag is free since the scan: the buckets)
        }
    }
}

__global__ __launch_bounds__(PV_THREADS) void vox_gather_kernel(VoxArgs a) {   // one wave per voxel row
    const int lane = threadIdx.x & 63;
    const int wave = (blockIdx.x * PV_THREADS + threadIdx.x) >> 6, nwaves = gridDim.x * (PV_THREADS / 64);
    for (int v = wave; v < a.B * a.MV; v += nwaves) {
        const int b = v / a.MV;
        if (v - b * a.MV >= a.voxel_num[b]) continue;
        const int s0 = a.start[v], c = a.start[v + 1] - s0;
        if (s0 < 0 || c < 0 || s0 + c > a.N) continue;
        if (lane == 0) a.num_points[v] = c < a.MP ? c : a.MP;
        const int *bk = a.flag + s0;
        for (int e = lane; e < c; e += 64) {
            const int idx = bk[e];
            int slot = 0;                       // position of idx in index order
            for (int j = 0; j < c; ++j) slot += bk[j] < idx;
            if (slot < a.MP) {
                const float *src = a.points + (size_t)idx * a.F;
                float *dst = a.voxels + ((size_t)v * a.MP + slot) * a.F;
                for (int k = 0; k < a.F; ++k) dst[k] = src[k];
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------ pillar encoder
constexpr int PE_WAVES = 4;            // waves per workgroup
constexpr int PE_MAX_POINTS = 64;      // rows of a voxel the LDS slab holds

struct EncArgs {
    const float *voxels;     // [B, MV, MP, F]
    const int *num_points;   // [B, MV]
    const int *coors;        // [B, MV, 4]
    const int *voxel_num;    // [B]
    const float *w1, *b1;    // [C1, F + 5], [C1]
    const float *w2, *b2;    // [64, 64], [64] (two layers)
    uint16_t *canvas;        // [B, H, W, 64]
    int B, MV, MP, H, W;
    float vx, vy, x_off, y_off;
};

template <int F, bool TWO>
__global__ __launch_bounds__(PE_WAVES * 64, 2) void pillar_encode_kernel(EncArgs a) {
    constexpr int K = F + 5;
    constexpr int C1 = TWO ? 32 : 64;
    constexpr int ROWS = PE_MAX_POINTS + 2;                 // + the padded row and the row maximum
    __shared__ __attribute__((aligned(16))) float s_pts[PE_WAVES][PE_MAX_POINTS * F];
    __shared__ __attribute__((aligned(16))) float s_x1[PE_WAVES][TWO ? ROWS * 32 : 4];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    float *pts = s_pts[wv];
    float *x1 = s_x1[wv];
    const int c1 = lane & (C1 - 1);
    const int half = TWO ? lane >> 5 : 0;                   // two layers: the two halves of the wave take alternate rows of layer 1

    __shared__ float s_w2t[TWO ? 32 * 64 : 1];            // w2[c][32 + k] at [k][c]: the half of layer 2 that meets the row maximum, once per voxel
    float w1[K], w2[TWO ? 32 : 1];                          // w2[c][0 .. 31]: the half that meets every row
#pragma unroll
    for (int k = 0; k < K; ++k) w1[k] = a.w1[c1 * K + k];
    const float sh1 = a.b1[c1];
    const float pad1 = fmaxf(sh1, 0.f);                     // what a padded (all-zero) row gives in layer 1
    float sh2 = 0.f;
    if (TWO) {
#pragma unroll
        for (int k = 0; k < 32; ++k) w2[k] = a.w2[lane * 64 + k];
        for (int e = threadIdx.x; e < 32 * 64; e += PE_WAVES * 64) s_w2t[e] = a.w2[(e & 63) * 64 + 32 + (e >> 6)];
        sh2 = a.b2[lane];
        if (lane < 32) x1[PE_MAX_POINTS * 32 + lane] = pad1;   // the padded row, the same for every voxel
        __syncthreads();                                    // s_w2t; the only workgroup barrier, before any wave leaves
    }

    const int wave = blockIdx.x * PE_WAVES + wv, nwaves = gridDim.x * PE_WAVES;
    for (int v = wave; v < a.B * a.MV; v += nwaves) {
        const int bv = v / a.MV;
        if (v - bv * a.MV >= a.voxel_num[bv]) continue;       // wave-uniform
        const int *co = a.coors + (size_t)v * 4;
        const int cb = co[0], cy = co[2], cx = co[3];
        if (cb < 0 || cb >= a.B || cy < 0 || cy >= a.H || cx < 0 || cx >= a.W) continue;
        uint16_t *dst = a.canvas + (((size_t)cb * a.H + cy) * a.W + cx) * 64 + lane;
        int n = a.num_points[v];
        n = n > a.MP ? a.MP : n;
        if (n <= 0) {                                       // the voxel mask (num_points > 0) zeroes the normalised rows: the output is zero
            *dst = 0;
            continue;
        }
        MD_WAVE_LDS_ORDER();                                // the previous voxel's reads are done before its slab is rewritten
        const float *src = a.voxels + (size_t)v * a.MP * F;
        for (int e = lane; e < n * F; e += 64) pts[e] = src[e];
        MD_WAVE_LDS_ORDER();
        // mean over the voxel's points: the sum in row order, then one divide
        float sx = 0.f, sy = 0.f, sz = 0.f;
#pragma unroll 1
        for (int r = 0; r < n; ++r) {
            sx = __fadd_rn(sx, pts[r * F]);
            sy = __fadd_rn(sy, pts[r * F + 1]);
            sz = __fadd_rn(sz, pts[r * F + 2]);
        }
        const float fn = (float)n;
        const float mx = __fdiv_rn(sx, fn), my = __fdiv_rn(sy, fn), mz = __fdiv_rn(sz, fn);
        const float ctr_x = __fadd_rn(__fmul_rn((float)cx, a.vx), a.x_off);
        const float ctr_y = __fadd_rn(__fmul_rn((float)cy, a.vy), a.y_off);

        float best = 0.f;                                   // ReLU outputs are >= 0
#pragma unroll 1
        for (int r = half; r < n; r += (TWO ? 2 : 1)) {
            float f[K];
#pragma unroll
            for (int k = 0; k < F; ++k) f[k] = pts[r * F + k];
            f[F] = __fsub_rn(f[0], mx);
            f[F + 1] = __fsub_rn(f[1], my);
            f[F + 2] = __fsub_rn(f[2], mz);
            f[F + 3] = __fsub_rn(f[0], ctr_x);
            f[F + 4] = __fsub_rn(f[1], ctr_y);
            float acc = 0.f;
#pragma unroll
            for (int k = 0; k < K; ++k) acc = fmaf(w1[k], f[k], acc);
            const float y = fmaxf(__fadd_rn(acc, sh1), 0.f);
            best = fmaxf(best, y);
            if (TWO) x1[r * 32 + c1] = y;
        }
        if (TWO) best = fmaxf(best, __shfl_xor(best, 32, 64));
        if (n < a.MP) best = fmaxf(best, pad1);             // the padded rows take part in the maximum
        if (!TWO) {
            *dst = f2bf_finite(best);
            continue;
        }
        if (lane < 32) x1[(PE_MAX_POINTS + 1) * 32 + lane] = best;
        MD_WAVE_LDS_ORDER();
        // layer 2, lane = output channel: input row = [x1 row (32), row maximum (32)]; the second half is the same for every row
        float tail = 0.f;
        {
            const float4 *m = (const float4 *)(x1 + (PE_MAX_POINTS + 1) * 32);
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const float4 t = m[q];
                tail = fmaf(s_w2t[(4 * q) * 64 + lane], t.x, tail);
                tail = fmaf(s_w2t[(4 * q + 1) * 64 + lane], t.y, tail);
                tail = fmaf(s_w2t[(4 * q + 2) * 64 + lane], t.z, tail);
                tail = fmaf(s_w2t[(4 * q + 3) * 64 + lane], t.w, tail);
            }
        }
        float best2 = 0.f;
        const int rows = n < a.MP ? n + 1 : n;              // + the padded row, once
#pragma unroll 1
        for (int r = 0; r < rows; ++r) {
            const float4 *xr = (const float4 *)(x1 + (r < n ? r : PE_MAX_POINTS) * 32);
            float acc = 0.f;
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const float4 t = xr[q];
                acc = fmaf(w2[4 * q], t.x, acc);
                acc = fmaf(w2[4 * q + 1], t.y, acc);
                acc = fmaf(w2[4 * q + 2], t.z, acc);
                acc = fmaf(w2[4 * q + 3], t.w, acc);
            }
            best2 = fmaxf(best2, fmaxf(__fadd_rn(__fadd_rn(acc, tail), sh2), 0.f));
        }
        *dst = f2bf_finite(best2);
    }
}

static inline bool finite_f(float x) { return x == x && x - x == 0.f; }

}  // namespace md

using namespace md;

// scratch of md_voxelize for N points and B samples of `cells` cells and MV voxels: eight i32 arrays, each padded to 64 entries.  The
// offsets count i32 entries, total counts bytes.  first, cvox: [B cells]; cell, flag: [N]; pre: [N + 1]; cnt: [B MV]; start: [B MV + 1];
// bsum: one entry per scan block of the longer of the two scans, and one more
struct VoxScratch { int64_t first, cvox, cell, flag, pre, cnt, start, bsum, total; };
static VoxScratch voxelize_scratch(Sz N, Sz B, Sz cells, Sz MV) {
    const Sz nbN = (N + (PV_BLOCK - 1)) / PV_BLOCK, nbV = (B * MV + (PV_BLOCK - 1)) / PV_BLOCK;
    Sz ints = 0;
    auto take = [&](Sz n) { const Sz at = ints; ints = ints + (n + 63) / 64 * 64; return (int64_t)at; };
    VoxScratch w;
    w.first = take(B * cells); w.cvox = take(B * cells);
    w.cell = take(N); w.flag = take(N); w.pre = take(N + 1);
    w.cnt = take(B * MV); w.start = take(B * MV + 1);
    w.bsum = take((nbN > nbV ? nbN : nbV) + 1);
    w.total = (int64_t)(ints * 4);
    return w;
}
extern "C" int64_t md_voxelize_workspace_bytes(int64_t N, int64_t B, int64_t cells, int64_t max_voxels) {
    return any_negative({N, B, cells, max_voxels}) ? -1 : ws_answer(voxelize_scratch(N, B, cells, max_voxels).total);
}

// in : points[N,F] f32, offsets[B+1] i32 ; out: voxels[B,MV,MP,F] f32, coors[B,MV,4] i32, num_points[B,MV] i32, voxel_num[B] i32
// [, workspace u8].  extra: md_voxelize_attrs (required).  Every check precedes the first device call.
extern "C" int md_voxelize(MD_AOT_ARGS) {
    Args g(MD_ARGS, 6, 7);
    const md_voxelize_attrs *at = g.attrs<md_voxelize_attrs>(extra);
    g.tensor(0, F32, 2); g.tensor(1, I32, 1); g.tensor(2, F32, 4); g.tensor(3, I32, 3); g.tensor(4, I32, 2); g.tensor(5, I32, 1);
    g.scratch(6);
    if (int rc = g.rc()) return rc;
    const int64_t N = g.d(0, 0), F = g.d(0, 1), B = g.d(1, 0) - 1;
    const int64_t MV = g.d(2, 1), MP = g.d(2, 2);
    if (F != 4 && F != 5) return MD_ERR_ARG;
    if (B < 0 || N < 0 || MV < 0 || MP < 0) return MD_ERR_ARG;
    if (g.d(2, 0) != B || g.d(2, 3) != F || g.d(3, 0) != B || g.d(3, 1) != MV || g.d(3, 2) != 4 || g.d(4, 0) != B || g.d(4, 1) != MV ||
        g.d(5, 0) != B)
        return MD_ERR_ARG;
    if (at->max_points != MP || at->max_voxels != MV) return MD_ERR_ARG;
    int grid[3];
    for (int k = 0; k < 3; ++k) {
        const float lo = at->range[k], hi = at->range[k + 3], vs = at->voxel_size[k];
        if (!finite_f(lo) || !finite_f(hi) || !finite_f(vs) || !(vs > 0.f) || !(hi > lo)) return MD_ERR_ARG;
        const float span = hi - lo;                          // the reference's fp32 (hi - lo) / vs, rounded half to even
        const float r = nearbyintf(span / vs);
        if (!(r >= 1.f) || r > 65536.f) return MD_ERR_ARG;
        grid[k] = (int)r;
    }
    const long long G = (long long)grid[0] * grid[1] * grid[2];
    if (N >= (1 << 30) || mul({G, B > 0 ? B : 1}) >= (1 << 30) || mul({B, MV}) >= (1 << 30) || B > 4096) return MD_ERR_SIZE;
    if (MP > 65536) return MD_ERR_SIZE;
    if (B == 0) return MD_OK;
    if (!g.have({0, 1, 2, 3, 4, 5})) return MD_ERR_ARG;

    const size_t nbN = (size_t)(N + PV_BLOCK - 1) / PV_BLOCK, nbV = (size_t)(B * MV + PV_BLOCK - 1) / PV_BLOCK;
    const size_t n_first = (size_t)(B * G), n_pts = (size_t)N, n_vox = (size_t)(B * MV);
    const VoxScratch w = voxelize_scratch(N, B, G, MV);
    hipStream_t s = (hipStream_t)stream;
    Scratch sc;
    if (int rc = sc.acquire((size_t)w.total, g, 6, s)) return rc;
    int *ws = (int *)sc.ptr;

    VoxArgs a;
    a.points = g.ptr<const float>(0); a.offsets = g.ptr<const int>(1);
    a.voxels = g.ptr<float>(2); a.coors = g.ptr<int>(3); a.num_points = g.ptr<int>(4); a.voxel_num = g.ptr<int>(5);
    a.N = (int)N; a.F = (int)F; a.B = (int)B; a.MV = (int)MV; a.MP = (int)MP;
    a.gx = grid[0]; a.gy = grid[1]; a.gz = grid[2]; a.G = (int)G;
    for (int k = 0; k < 3; ++k) { a.lo[k] = at->range[k]; a.vs[k] = at->voxel_size[k]; }
    a.first = ws + w.first; a.cell_vox = ws + w.cvox; a.cell_of = ws + w.cell; a.flag = ws + w.flag; a.pre = ws + w.pre;
    a.cnt = ws + w.cnt; a.start = ws + w.start; a.bsum = ws + w.bsum;

    if (n_vox * MP * F) MD_HIP_TRY(hipMemsetAsync(a.voxels, 0, n_vox * MP * F * 4, s));
    if (n_vox) MD_HIP_TRY(hipMemsetAsync(a.coors, 0, n_vox * 16, s));
    if (n_vox) MD_HIP_TRY(hipMemsetAsync(a.num_points, 0, n_vox * 4, s));
    MD_HIP_TRY(hipMemsetAsync(a.voxel_num, 0, (size_t)B * 4, s));
    if (N == 0 || MV == 0 || MP == 0) return MD_OK;
    MD_HIP_TRY(hipMemsetAsync(a.first, 0x7f, n_first * 4, s));   // 0x7f7f7f7f: above every point index (N < 2^30)
    MD_HIP_TRY(hipMemsetAsync(a.cnt, 0, n_vox * 4, s));
    const unsigned gp = grid1d(n_pts);
    hipLaunchKernelGGL(vox_cell_kernel, dim3(gp), dim3(PV_THREADS), 0, s, a);
    hipLaunchKernelGGL(vox_flag_kernel, dim3(gp), dim3(PV_THREADS), 0, s, a);
    hipLaunchKernelGGL(scan_reduce_kernel, dim3((unsigned)nbN), dim3(PV_THREADS), 0, s, (const int *)a.flag, a.N, a.bsum);
    hipLaunchKernelGGL(scan_top_kernel, dim3(1), dim3(PV_THREADS), 0, s, a.bsum, (int)nbN);
    hipLaunchKernelGGL(scan_down_kernel, dim3((unsigned)nbN), dim3(PV_THREADS), 0, s, (const int *)a.flag, a.N, (const int *)a.bsum, a.pre);
    hipLaunchKernelGGL(vox_rank_kernel, dim3(gp), dim3(PV_THREADS), 0, s, a);
    hipLaunchKernelGGL(vox_count_kernel, dim3(gp), dim3(PV_THREADS), 0, s, a);
    hipLaunchKernelGGL(scan_reduce_kernel, dim3((unsigned)nbV), dim3(PV_THREADS), 0, s, (const int *)a.cnt, (int)n_vox, a.bsum);
    hipLaunchKernelGGL(scan_top_kernel, dim3(1), dim3(PV_THREADS), 0, s, a.bsum, (int)nbV);
    hipLaunchKernelGGL(scan_down_kernel, dim3((unsigned)nbV), dim3(PV_THREADS), 0, s, (const int *)a.cnt, (int)n_vox, (const int *)a.bsum,
                       a.start);
    hipLaunchKernelGGL(vox_fill_kernel, dim3(gp), dim3(PV_THREADS), 0, s, a);
    hipLaunchKernelGGL(vox_gather_kernel, dim3(grid1d(n_vox * 64)), dim3(PV_THREADS), 0, s, a);
    return launched();
}

// in : voxels[B,MV,MP,F] f32, num_points[B,MV] i32, coors[B,MV,4] i32, voxel_num[B] i32, w1[C1,F+5] f32, b1[C1] f32,
//      w2[64,64] f32 or NULL, b2[64] f32 or NULL ; out: canvas[B,H,W,64] bf16.  extra: md_pillar_encode_attrs (required).
extern "C" int md_pillar_encode(MD_AOT_ARGS) {
    Args g(MD_ARGS, 9, 9);
    const md_pillar_encode_attrs *at = g.attrs<md_pillar_encode_attrs>(extra);
    g.tensor(0, F32, 4); g.tensor(1, I32, 2); g.tensor(2, I32, 3); g.tensor(3, I32, 1); g.tensor(4, F32, 2); g.tensor(5, F32, 1);
    g.optional(6, F32, 2); g.optional(7, F32, 1); g.tensor(8, BF16, 4);
    if (int rc = g.rc()) return rc;
    if (at->with_distance != 0 || at->virtual_points != 0) return MD_ERR_ARG;
    if (!finite_f(at->vx) || !finite_f(at->vy) || !finite_f(at->x_offset) || !finite_f(at->y_offset)) return MD_ERR_ARG;
    const int64_t B = g.d(0, 0), MV = g.d(0, 1), MP = g.d(0, 2), F = g.d(0, 3);
    const int64_t H = g.d(8, 1), W = g.d(8, 2);
    if (F != 4 && F != 5) return MD_ERR_ARG;
    const bool two = g.given(6);
    if (two != g.given(7)) return MD_ERR_ARG;
    const int64_t C1 = two ? 32 : 64;
    if (g.d(1, 0) != B || g.d(1, 1) != MV || g.d(2, 0) != B || g.d(2, 1) != MV || g.d(2, 2) != 4 || g.d(3, 0) != B) return MD_ERR_ARG;
    if (g.d(4, 0) != C1 || g.d(4, 1) != F + 5 || g.d(5, 0) != C1) return MD_ERR_ARG;   // other widths are not built
    if (two && (g.d(6, 0) != 64 || g.d(6, 1) != 64 || g.d(7, 0) != 64)) return MD_ERR_ARG;
    if (g.d(8, 0) != B || g.d(8, 3) != 64 || H < 0 || W < 0 || B < 0 || MV < 0 || MP < 0) return MD_ERR_ARG;
    if (MP > PE_MAX_POINTS) return MD_ERR_SIZE;
    if (mul({B, MV}) >= (1 << 30) || !fits_i32(mul({B, MV, MP, F}) / 4) || H > 65536 || W > 65536 || !fits_i32(mul({B, H, W}) / 4))
        return MD_ERR_SIZE;
    if (B * H * W == 0) return MD_OK;
    if (!g.have({0, 1, 2, 3, 4, 5, 8})) return MD_ERR_ARG;
    EncArgs a;
    a.voxels = g.ptr<const float>(0); a.num_points = g.ptr<const int>(1); a.coors = g.ptr<const int>(2); a.voxel_num = g.ptr<const int>(3);
    a.w1 = g.ptr<const float>(4); a.b1 = g.ptr<const float>(5);
    a.w2 = two ? g.ptr<const float>(6) : nullptr; a.b2 = two ? g.ptr<const float>(7) : nullptr;
    a.canvas = g.ptr<uint16_t>(8);
    a.B = (int)B; a.MV = (int)MV; a.MP = (int)MP; a.H = (int)H; a.W = (int)W;
    a.vx = at->vx; a.vy = at->vy; a.x_off = at->x_offset; a.y_off = at->y_offset;
    hipStream_t s = (hipStream_t)stream;
    MD_HIP_TRY(hipMemsetAsync(a.canvas, 0, (size_t)(B * H * W) * 64 * 2, s));   // cells without a pillar are zero
    if (B * MV == 0 || MP == 0) return MD_OK;
    void (*k)(EncArgs) = F == 5 ? (two ? pillar_encode_kernel<5, true> : pillar_encode_kernel<5, false>)
                                : (two ? pillar_encode_kernel<4, true> : pillar_encode_kernel<4, false>);
    const size_t wgs = (size_t)(B * MV + PE_WAVES - 1) / PE_WAVES;
    hipLaunchKernelGGL(k, dim3((unsigned)(wgs < 2048 ? wgs : 2048)), dim3(PE_WAVES * 64), 0, s, a);
    return launched();
}
