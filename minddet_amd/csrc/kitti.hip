// kitti.hip -- the camera-frame ends of the KITTI PointPillars path on the device (include/minddet_hip_kitti.h): the cut of a raw scan
// to convex hulls (the image frustum of remove_outside_points, the frustums of reference_detections) in front of md_voxelize and
// md_pc_augment_points (pillars.hip, pcaug.hip), the label boxes from the camera frame to the lidar frame, and the KITTI result rows
// behind md_pp_decode_selected (pphead.hip).
//
// md_pc_crop_hulls: four launches, no memset, nothing read back.
//   kc_planes_kernel    one lane per surface: the [B,K,6,4] float64 planes of surface_equ_3d_jit, into the workspace
//   kc_classify_kernel  256 points per workgroup: the planes of the sample of the workgroup's first point staged in LDS (12 KiB at
//                       K = 64); a lane whose point lies in a later sample (a workgroup may straddle samples) reads its planes from
//                       the workspace instead.  A hull is left at its first non-negative sign, the hulls at the first that holds the
//                       point.  keep[i] and the workgroup's count (block_keep_count)
//   kc_scan_kernel      one workgroup: the prefix of the counts (compaction_offsets); offsets_out[b] = the kept points before offsets[b]
//   kc_scatter_kernel   ballot ranks (block_rank) from keep[], the row copied once; the zero rows from the total on
// md_kitti_boxes_to_lidar: one lane per label row.  md_kitti_rows: one wave per sample, 64 detections at a time, ballot ranks.
// Float64 without contraction: every sum is the contract's sum (tests/kitti_io_contract.py), term by term.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "aot.h"
#include "../../include/minddet_hip_kitti.h"

#pragma clang fp contract(off)

#include "aug_geom.h"
#include "workgroup.h"

namespace md {

static_assert(sizeof(md_kitti_rows_attrs) == 32, "minddet_hip_kitti.h: attribute struct layout");

constexpr const char *F64 = "float64";
constexpr int KC_MAX_HULLS = MD_CROP_MAX_HULLS;
constexpr int KC_PLANE = 24;      // doubles per hull: six surfaces of (n0, n1, n2, d)

struct CropArgs {
    const float4 *pts; const int *offsets; const double *hulls; const int *hull_count;
    float4 *out; int *offsets_out; uint8_t *keep;
    double *planes; int *bsum;
    int N, B, K, nb;
};

// corner_to_surfaces_3d_jit's table (box_np_ops.py:735-737), the first three corners of each surface
__constant__ int kc_surface[6][3] = {{0, 1, 2}, {7, 6, 5}, {0, 3, 7}, {1, 5, 6}, {0, 4, 5}, {3, 2, 6}};

__global__ __launch_bounds__(256) void kc_planes_kernel(CropArgs a) {
    const int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (id >= (int64_t)a.B * a.K * 6) return;
    const int j = (int)(id % 6);
    const double *c = a.hulls + (size_t)(id / 6) * 24;
    const double *s0 = c + 3 * kc_surface[j][0], *s1 = c + 3 * kc_surface[j][1], *s2 = c + 3 * kc_surface[j][2];
    const double ax = s0[0] - s1[0], ay = s0[1] - s1[1], az = s0[2] - s1[2];
    const double bx = s1[0] - s2[0], by = s1[1] - s2[1], bz = s1[2] - s2[2];
    const double n0 = ay * bz - az * by, n1 = az * bx - ax * bz, n2 = ax * by - ay * bx;      // np.cross
    double *o = a.planes + (size_t)id * 4;
    o[0] = n0; o[1] = n1; o[2] = n2;
    o[3] = -((n0 * s0[0] + n1 * s0[1]) + n2 * s0[2]);
}

__device__ __forceinline__ bool inside_hull(const double *pl, double x, double y, double z) {
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        const double sign = ((x * pl[4 * j] + y * pl[4 * j + 1]) + z * pl[4 * j + 2]) + pl[4 * j + 3];
        if (sign >= 0) return false;
    }
    return true;
}

__global__ __launch_bounds__(256) void kc_classify_kernel(CropArgs a) {
    __shared__ double lds[KC_MAX_HULLS * KC_PLANE];
    __shared__ int wcnt[4];
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int b0 = find_sample(a.offsets, a.B, blockIdx.x * 256);                  // uniform
    if (b0 >= 0) {
        const int n0 = min(max(a.hull_count[b0], 0), a.K) * KC_PLANE;
        const double *src = a.planes + (size_t)b0 * a.K * KC_PLANE;
        for (int e = threadIdx.x; e < n0; e += 256) lds[e] = src[e];
    }
    __syncthreads();
    const int b = find_sample(a.offsets, a.B, i);
    bool keep = false;
    if (i < a.N && b >= 0) {
        const float4 p = a.pts[i];
        const double x = p.x, y = p.y, z = p.z;
        const int cnt = min(max(a.hull_count[b], 0), a.K);
        const double *pl = b == b0 ? lds : a.planes + (size_t)b * a.K * KC_PLANE;
        for (int k = 0; k < cnt && !keep; ++k) keep = inside_hull(pl + k * KC_PLANE, x, y, z);
    }
    if (i < a.N) a.keep[i] = keep ? 1 : 0;
    block_keep_count(keep, wcnt, a.bsum);
}

__global__ __launch_bounds__(256) void kc_scan_kernel(CropArgs a) {
    __shared__ int wsum[4];
    compaction_offsets(a.bsum, a.nb, wsum);
    for (int b = threadIdx.x; b <= a.B; b += 256) {
        const int o = min(max(a.offsets[b], 0), a.N), blk = o >> 8;      // blk <= nb
        int v = a.bsum[blk];
        for (int k = blk << 8; k < o; ++k) v += a.keep[k] != 0;
        a.offsets_out[b] = v;
    }
}

__global__ __launch_bounds__(256) void kc_scatter_kernel(CropArgs a) {
    __shared__ int wcnt[4];
    const int i = blockIdx.x * 256 + threadIdx.x;
    const bool keep = i < a.N && a.keep[i] != 0;
    const int at = block_rank(keep, wcnt, a.bsum);
    const int total = a.bsum[a.nb];
    if (i < a.N && i >= total) a.out[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (keep && at >= 0 && at < a.N) a.out[at] = a.pts[i];
}

struct LidarArgs {
    const float *cam; const int *count; const double *m;
    float *out;
    int B, G;
};

__global__ __launch_bounds__(256) void kb_to_lidar_kernel(LidarArgs a) {
    const int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (id >= (int64_t)a.B * a.G) return;
    const int b = (int)(id / a.G), g = (int)(id % a.G);
    float *o = a.out + (size_t)id * 7;
    if (g >= min(max(a.count[b], 0), a.G)) {
        for (int e = 0; e < 7; ++e) o[e] = 0.f;
        return;
    }
    const float *q = a.cam + (size_t)id * 7;
    const double *m = a.m + (size_t)b * 16;
    const double x = q[0], y = q[1], z = q[2];
    for (int r = 0; r < 3; ++r) o[r] = (float)(((m[4 * r] * x + m[4 * r + 1] * y) + m[4 * r + 2] * z) + m[4 * r + 3]);
    o[3] = q[5]; o[4] = q[3]; o[5] = q[4]; o[6] = q[6];
}

struct RowArgs {
    const float *dets; const int *count; const double *l2c, *p2; const int *shape;
    float *rows; int *src, *out_count;
    int M, use_limit, lidar_input;
    double lim[6];
};

// numpy's min / max over an axis: a NaN stays
__device__ __forceinline__ double np_min(double m, double v) { return (v < m || v != v) ? v : m; }
__device__ __forceinline__ double np_max(double m, double v) { return (v > m || v != v) ? v : m; }

__global__ __launch_bounds__(64) void kr_rows_kernel(RowArgs a) {
    const int b = blockIdx.x, lane = threadIdx.x, M = a.M;
    const int cnt = min(max(a.count[b], 0), M);
    const double *L = a.l2c + (size_t)b * 16, *P = a.p2 + (size_t)b * 16;
    const double H = (double)a.shape[2 * b], W = (double)a.shape[2 * b + 1];
    int base = 0;
    for (int m0 = 0; m0 < cnt; m0 += 64) {
        const int m = m0 + lane;
        bool keep = false;
        float o[14];
        if (m < cnt) {
            const float *q = a.dets + ((size_t)b * M + m) * 9;
            const double x = q[0], y = q[1], z = q[2], w = q[3], l = q[4], h = q[5], r = q[6];
            double loc[3];
            for (int e = 0; e < 3; ++e) loc[e] = ((L[4 * e] * x + L[4 * e + 1] * y) + L[4 * e + 2] * z) + L[4 * e + 3];
            double s, c;
            sincos(r, &s, &c);
            const double hl = l / 2, hw = w / 2;
            const double sx[8] = {1, 1, -1, -1, 1, 1, -1, -1}, sz[8] = {1, -1, -1, 1, 1, -1, -1, 1};
            double x1 = 0, y1 = 0, x2 = 0, y2 = 0;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const double xc = sx[k] * hl, zc = sz[k] * hw, yc = k < 4 ? 0.0 : -h;
                const double X = (xc * c + zc * s) + loc[0], Y = yc + loc[1], Z = (-xc * s + zc * c) + loc[2];
                const double u = (((P[0] * X + P[1] * Y) + P[2] * Z) + P[3]) / Z;
                const double v = (((P[4] * X + P[5] * Y) + P[6] * Z) + P[7]) / Z;
                if (k == 0) { x1 = x2 = u; y1 = y2 = v; }
                else { x1 = np_min(x1, u); y1 = np_min(y1, v); x2 = np_max(x2, u); y2 = np_max(y2, v); }
            }
            keep = true;
            if (!a.lidar_input && (x1 > W || y1 > H || x2 < 0 || y2 < 0)) keep = false;
            if (a.use_limit && (x < a.lim[0] || y < a.lim[1] || z < a.lim[2] || x > a.lim[3] || y > a.lim[4] || z > a.lim[5])) keep = false;
            if (W < x2) x2 = W;
            if (H < y2) y2 = H;
            if (0 > x1) x1 = 0;
            if (0 > y1) y1 = 0;
            o[0] = (float)(-atan2(-y, x) + r);
            o[1] = (float)x1; o[2] = (float)y1; o[3] = (float)x2; o[4] = (float)y2;
            o[5] = q[4]; o[6] = q[5]; o[7] = q[3];
            o[8] = (float)loc[0]; o[9] = (float)loc[1]; o[10] = (float)loc[2];
            o[11] = q[6]; o[12] = q[7]; o[13] = q[8];
        }
        const unsigned long long bal = __ballot(keep);
        if (keep) {
            const int at = base + lane_rank(bal);
            float *dst = a.rows + ((size_t)b * M + at) * 14;
            for (int e = 0; e < 14; ++e) dst[e] = o[e];
            a.src[(size_t)b * M + at] = m;
        }
        base += __popcll(bal);
    }
    for (int m = base + lane; m < M; m += 64) {
        float *dst = a.rows + ((size_t)b * M + m) * 14;
        for (int e = 0; e < 14; ++e) dst[e] = 0.f;
        a.src[(size_t)b * M + m] = -1;
    }
    if (lane == 0) a.out_count[b] = base;
}

}  // namespace md

using namespace md;

// scratch of md_pc_crop_hulls: planes[B K][KC_PLANE] f64 at 0, bsum[ceil(N / 256) + 1] i32
struct CropScratch { int64_t bsum, total; };
static CropScratch crop_scratch(Sz N, Sz B, Sz K) {
    const Sz bsum = B * K * KC_PLANE * 8, total = bsum + ((N + 255) / 256 + 1) * 4;
    return {(int64_t)bsum, (int64_t)total};
}
extern "C" int64_t md_pc_crop_hulls_workspace_bytes(int64_t N, int64_t B, int64_t K) {
    return any_negative({N, B, K}) ? -1 : ws_answer(crop_scratch(N, B, K).total);
}

extern "C" int md_pc_crop_hulls(MD_AOT_ARGS) {
    // in : points[N,4] f32, offsets[B+1] i32, hulls[B,K,8,3] f64, hull_count[B] i32
    // out: points_out[N,4] f32, offsets_out[B+1] i32, keep[N] u8 ; [workspace]
    Args a(MD_ARGS, 7, 8);
    a.tensor(0, F32, 2); a.tensor(1, I32, 1); a.tensor(2, F64, 4); a.tensor(3, I32, 1);
    a.tensor(4, F32, 2); a.tensor(5, I32, 1); a.tensor(6, U8, 1); a.scratch(7);
    if (int rc = a.rc()) return rc;
    const int64_t N = a.d(0, 0), B = a.d(1, 0) - 1, K = a.d(2, 1);
    a.require(N >= 0 && B >= 0 && K >= 0 && a.d(0, 1) == 4 && a.d(2, 0) == B && a.d(2, 2) == 8 && a.d(2, 3) == 3 && a.d(3, 0) == B);
    a.require(a.same_shape(4, 0) && a.same_shape(5, 1) && a.d(6, 0) == N);
    if (int rc = a.rc()) return rc;
    if (N >= ((int64_t)1 << 30) || K > KC_MAX_HULLS || B > MD_CROP_MAX_BATCH) return MD_ERR_SIZE;
    if (!a.have({1, 5})) return MD_ERR_ARG;
    if (B > 0 && !a.have({3})) return MD_ERR_ARG;
    if (B * K > 0 && !a.have({2})) return MD_ERR_ARG;
    if (N > 0 && !a.have({0, 4, 6})) return MD_ERR_ARG;
    if (aliased(params, 4, 7)) return MD_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    const int64_t nb = (N + 255) / 256;
    const CropScratch w = crop_scratch(N, B, K);
    Scratch ws;
    if (int rc = ws.acquire((size_t)w.total, a, 7, s)) return rc;
    CropArgs k;
    k.pts = (const float4 *)params[0]; k.offsets = (const int *)params[1]; k.hulls = (const double *)params[2];
    k.hull_count = (const int *)params[3];
    k.out = (float4 *)params[4]; k.offsets_out = (int *)params[5]; k.keep = (uint8_t *)params[6];
    k.planes = (double *)ws.ptr; k.bsum = (int *)((char *)ws.ptr + w.bsum);
    k.N = (int)N; k.B = (int)B; k.K = (int)K; k.nb = (int)nb;
    if (B * K > 0) hipLaunchKernelGGL(kc_planes_kernel, dim3((unsigned)((B * K * 6 + 255) / 256)), dim3(256), 0, s, k);
    if (nb > 0) hipLaunchKernelGGL(kc_classify_kernel, dim3((unsigned)nb), dim3(256), 0, s, k);
    hipLaunchKernelGGL(kc_scan_kernel, dim3(1), dim3(256), 0, s, k);
    if (nb > 0) hipLaunchKernelGGL(kc_scatter_kernel, dim3((unsigned)nb), dim3(256), 0, s, k);
    return launched();
}

extern "C" int md_kitti_boxes_to_lidar(MD_AOT_ARGS) {
    // in : boxes_cam[B,G,7] f32, gt_count[B] i32, cam2lidar[B,4,4] f64
    // out: boxes_lidar[B,G,7] f32
    Args a(MD_ARGS, 4, 4);
    a.tensor(0, F32, 3); a.tensor(1, I32, 1); a.tensor(2, F64, 3); a.tensor(3, F32, 3);
    if (int rc = a.rc()) return rc;
    const int64_t B = a.d(0, 0), G = a.d(0, 1);
    a.require(B >= 0 && G >= 0 && a.d(0, 2) == 7 && a.d(1, 0) == B && a.d(2, 0) == B && a.d(2, 1) == 4 && a.d(2, 2) == 4 && a.same_shape(3, 0));
    if (int rc = a.rc()) return rc;
    if (G > MD_KITTI_MAX_LABELS || B > MD_KITTI_MAX_BATCH) return MD_ERR_SIZE;
    if (B > 0 && !a.have({1, 2})) return MD_ERR_ARG;
    if (B * G > 0 && !a.have({0, 3})) return MD_ERR_ARG;
    if (aliased(params, 3, 4)) return MD_ERR_ARG;
    if (B * G == 0) return MD_OK;
    LidarArgs k;
    k.cam = (const float *)params[0]; k.count = (const int *)params[1]; k.m = (const double *)params[2]; k.out = (float *)params[3];
    k.B = (int)B; k.G = (int)G;
    hipLaunchKernelGGL(kb_to_lidar_kernel, dim3((unsigned)((B * G + 255) / 256)), dim3(256), 0, (hipStream_t)stream, k);
    return launched();
}

extern "C" int md_kitti_rows(MD_AOT_ARGS) {
    // in : dets[B,M,9] f32, count[B] i32, lidar2cam[B,4,4] f64, p2[B,4,4] f64, image_shape[B,2] i32
    // out: rows[B,M,14] f32, src[B,M] i32, out_count[B] i32
    Args a(MD_ARGS, 8, 8);
    const md_kitti_rows_attrs *at = a.attrs<md_kitti_rows_attrs>(extra);
    a.tensor(0, F32, 3); a.tensor(1, I32, 1); a.tensor(2, F64, 3); a.tensor(3, F64, 3); a.tensor(4, I32, 2);
    a.tensor(5, F32, 3); a.tensor(6, I32, 2); a.tensor(7, I32, 1);
    if (int rc = a.rc()) return rc;
    const int64_t B = a.d(0, 0), M = a.d(0, 1);
    a.require(B >= 0 && M >= 0 && a.d(0, 2) == 9 && a.d(1, 0) == B && a.d(2, 0) == B && a.d(2, 1) == 4 && a.d(2, 2) == 4 && a.same_shape(3, 2));
    a.require(a.d(4, 0) == B && a.d(4, 1) == 2 && a.d(5, 0) == B && a.d(5, 1) == M && a.d(5, 2) == 14 && a.d(6, 0) == B && a.d(6, 1) == M);
    a.require(a.d(7, 0) == B);
    a.require((at->use_limit == 0 || at->use_limit == 1) && (at->lidar_input == 0 || at->lidar_input == 1));
    if (at->use_limit == 1)
        for (int i = 0; i < 6; ++i) a.require(!isnan(at->limit_range[i]));
    if (int rc = a.rc()) return rc;
    if (M > MD_KITTI_MAX_DETS || B > MD_KITTI_MAX_BATCH) return MD_ERR_SIZE;
    if (B > 0 && !a.have({1, 2, 3, 4, 7})) return MD_ERR_ARG;
    if (B * M > 0 && !a.have({0, 5, 6})) return MD_ERR_ARG;
    if (aliased(params, 5, 8)) return MD_ERR_ARG;
    if (B == 0) return MD_OK;
    RowArgs k;
    k.dets = (const float *)params[0]; k.count = (const int *)params[1]; k.l2c = (const double *)params[2]; k.p2 = (const double *)params[3];
    k.shape = (const int *)params[4];
    k.rows = (float *)params[5]; k.src = (int *)params[6]; k.out_count = (int *)params[7];
    k.M = (int)M; k.use_limit = at->use_limit; k.lidar_input = at->lidar_input;
    for (int i = 0; i < 6; ++i) k.lim[i] = (double)at->limit_range[i];
    hipLaunchKernelGGL(kr_rows_kernel, dim3((unsigned)B), dim3(64), 0, (hipStream_t)stream, k);
    return launched();
}
